"""sample_moments of UnderdampedLangevin and GeneralizedHMC on the CPU: the eager route against the restatement of
kinetic_moments_cases.py bit for bit, the final states against sample(), the harmonic laws (the position marginal and BAOAB's
kinetic temperature), the stuck double well, validation, the routing of the fused call, the refusals of ebm_kinetic_moments_f32 in
front of any launch, and the generalized-HMC cases of test_kinetic_moments_gpu.py themselves (margins)."""

import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib
from torchebm_amd.samplers.moments import ChainMoments, recip_table
from helpers import fused_cpu  # noqa: F401
from kinetic_cases import law_bar
from kinetic_moments_cases import (GAMMA, GHMC_CASES, MARGIN_BAR, TEMP, energy_spec, ghmc_case, model_of, oracle_of, restate_baoab,
                                   restate_ghmc, two_pass, v2_mean, welford)

ENTRY = "ebm_kinetic_moments_f32"
H_BAOAB = {"double_well": 0.05, "harmonic": 0.3, "gaussian": 0.3}
EPS_GHMC = {"double_well": 0.15, "harmonic": 0.4, "gaussian": 0.4}
L_GHMC = 2


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _make(which, spec, kind):
    if which == "baoab":
        return ta.UnderdampedLangevin(model_of(spec), step_size=H_BAOAB[kind], friction=GAMMA, temperature=TEMP)
    return ta.GeneralizedHMC(model_of(spec), step_size=EPS_GHMC[kind], n_leapfrog_steps=L_GHMC, friction=GAMMA, temperature=TEMP)


def _replay(which, seed, n, dim, k):
    """The draws of the eager routes, in their order: the start velocities, then per transition randn(n, dim) and, for
    generalized HMC, rand(n)."""
    g = _gen(seed)
    xi0 = torch.randn(n, dim, generator=g)
    z, u = [], []
    for _ in range(k):
        z.append(torch.randn(n, dim, generator=g))
        if which == "ghmc":
            u.append(torch.rand(n, generator=g))
    return xi0, torch.stack(z), (torch.stack(u) if u else None)


# ---------------------------------------------------------------------------------
# the eager route against the restatement
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["baoab", "ghmc"])
@pytest.mark.parametrize("kind", ["double_well", "harmonic", "gaussian"])
@pytest.mark.parametrize("dim", [2, 5])
@pytest.mark.parametrize("n_steps,burn_in", [(11, 3), (12, 0)])
def test_eager_route_is_the_restatement_bit_for_bit(which, kind, dim, n_steps, burn_in):
    n, h = 9, (n_steps - burn_in) // 2
    spec = energy_spec(kind, dim)
    x0 = torch.randn(n, dim, generator=_gen(1))
    keep = x0.clone()
    xi0, z, u = _replay(which, 7, n, dim, n_steps)
    if which == "baoab":
        want = restate_baoab(oracle_of(spec), x0, None, z, H_BAOAB[kind], GAMMA, TEMP, burn_in, xi0=xi0)
    else:
        want = restate_ghmc(oracle_of(spec), x0, None, z, u, EPS_GHMC[kind], L_GHMC, GAMMA, TEMP, burn_in, xi0=xi0)
    x, mom, v = _make(which, spec, kind).sample_moments(x=x0, n_steps=n_steps, burn_in=burn_in, energy=True, return_velocity=True,
                                                        generator=_gen(7))
    assert torch.equal(x0, keep)
    assert torch.equal(x, want["x"]) and torch.equal(v, want["v"])
    mean, m2 = welford(want["traj"], h)
    assert torch.equal(mom.chain_mean, mean) and torch.equal(mom.chain_m2, m2)
    e_mean, e_m2 = welford(want["e_traj"], h)
    assert torch.equal(mom.energy_mean, e_mean) and torch.equal(mom.energy_m2, e_m2)
    assert mom.half_len == h and mom.n_nonfinite == 0
    if which == "baoab":
        assert mom.acceptance_rate is None
        assert torch.equal(mom.velocity_sq_mean, v2_mean(want["v_traj"], h))
        assert mom.kinetic_temperature.shape == (dim,) and mom.kinetic_temperature.dtype == torch.float64
        assert torch.allclose(mom.kinetic_temperature, want["v_traj"].double().square().mean(dim=(0, 1)), rtol=1e-6)
    else:
        assert mom.velocity_sq_mean is None and mom.kinetic_temperature is None
        assert torch.allclose(mom.acceptance_rate, want["accepted"].float().mean(dim=1))
    # the final states are sample()'s for the same seed
    xs, vs = _make(which, spec, kind).sample(x=x0, n_steps=n_steps, return_velocity=True, generator=_gen(7))
    assert torch.equal(x, xs) and torch.equal(v, vs)


@pytest.mark.parametrize("which", ["baoab", "ghmc"])
def test_a_passed_velocity_is_continued_and_never_written(which):
    spec = energy_spec("double_well", 3)
    x0, v0 = torch.randn(7, 3, generator=_gen(2)), torch.randn(7, 3, generator=_gen(3))
    keep = v0.clone()
    x, mom, v = _make(which, spec, "double_well").sample_moments(x=x0, n_steps=8, velocity=v0, return_velocity=True, generator=_gen(4))
    xs, vs = _make(which, spec, "double_well").sample(x=x0, n_steps=8, velocity=v0, return_velocity=True, generator=_gen(4))
    assert torch.equal(v0, keep) and torch.equal(x, xs) and torch.equal(v, vs) and mom.energy_mean is None
    out = _make(which, spec, "double_well").sample_moments(x=x0, n_steps=8, generator=_gen(4))
    assert len(out) == 2 and isinstance(out[1], ChainMoments)


# ---------------------------------------------------------------------------------
# the laws on a harmonic well
# ---------------------------------------------------------------------------------
LAW = dict(k=4.0, step=0.3, gamma=1.0, temp=1.0, n=4096, dim=4, n_steps=400, burn_in=100, seed=0)
LAW_GHMC_L = 3


def law_start(device=None):
    x0 = math.sqrt(LAW["temp"] / LAW["k"]) * torch.randn(LAW["n"], LAW["dim"], generator=_gen(LAW["seed"]))
    return x0 if device is None else x0.to(device)


def check_baoab_law(mom):
    """Pooled var k = 1 (BAOAB's position marginal is exact on a quadratic) and kinetic_temperature = T (1 - h^2 k / 4) = 0.91,
    each within 4.5 standard errors of the variance of n dim independent normal values, relative.  The bar counts the chains
    only as independent: time-averaging positively correlated draws cannot widen it."""
    bar = 4.5 * math.sqrt(2.0 / (LAW["n"] * LAW["dim"]))
    assert math.isclose(bar, 0.0497, abs_tol=1e-4)
    var_k = mom.var.cpu() * LAW["k"]
    kt = mom.kinetic_temperature.cpu() / 0.91
    print("baoab law: var k", var_k.tolist(), "kinetic_temperature / 0.91", kt.tolist(), "bar", bar, "max rhat", float(mom.rhat.max()))
    assert mom.n_nonfinite == 0
    assert ((var_k - 1.0).abs() < bar).all()
    assert ((kt - 1.0).abs() < bar).all()


def check_ghmc_law(mom):
    bar = 4.5 * math.sqrt(2.0 / (LAW["n"] * LAW["dim"]))
    var_k = mom.var.cpu() * LAW["k"]
    print("ghmc law: var k", var_k.tolist(), "bar", bar, "acceptance", float(mom.acceptance_rate.mean()), "max rhat", float(mom.rhat.max()))
    assert mom.n_nonfinite == 0 and mom.kinetic_temperature is None
    assert ((var_k - 1.0).abs() < bar).all()
    assert 0.5 < float(mom.acceptance_rate.mean()) < 1.0


def test_baoab_meets_the_harmonic_laws():
    s = ta.UnderdampedLangevin(ta.HarmonicModel(k=LAW["k"]), step_size=LAW["step"], friction=LAW["gamma"], temperature=LAW["temp"])
    _, mom = s.sample_moments(x=law_start(), n_steps=LAW["n_steps"], burn_in=LAW["burn_in"], generator=_gen(LAW["seed"]))
    assert math.isclose(1.0 - LAW["step"] ** 2 * LAW["k"] / 4.0, 0.91)
    check_baoab_law(mom)


def test_ghmc_meets_the_harmonic_law():
    s = ta.GeneralizedHMC(ta.HarmonicModel(k=LAW["k"]), step_size=LAW["step"], n_leapfrog_steps=LAW_GHMC_L, friction=LAW["gamma"],
                          temperature=LAW["temp"])
    _, mom = s.sample_moments(x=law_start(), n_steps=LAW["n_steps"], burn_in=LAW["burn_in"], generator=_gen(LAW["seed"]))
    check_ghmc_law(mom)


# ---------------------------------------------------------------------------------
# the stuck double well
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["baoab", "ghmc"])
def test_stuck_double_well_raises_the_alarm(which):
    """The run of test_moments.py under the two samplers: barrier 8, dim 2, half of the chains started in each well.  R-hat is
    well above 1 and is the float64 two-pass value of the run's own trajectory within the tolerance that test uses."""
    n = 512
    x0 = torch.ones(n, 2)
    x0[: n // 2] = -1.0
    model = lambda: ta.DoubleWellModel(barrier_height=8.0)  # noqa: E731
    if which == "baoab":
        make = lambda: ta.UnderdampedLangevin(model(), step_size=0.02)  # noqa: E731
    else:
        make = lambda: ta.GeneralizedHMC(model(), step_size=0.02, n_leapfrog_steps=3)  # noqa: E731
    _, mom = make().sample_moments(x=x0, n_steps=400, generator=_gen(3))
    print("stuck double well:", which, "rhat", mom.rhat.tolist(), "ess", mom.ess.tolist())
    assert (mom.rhat > 1.1).all()
    assert (mom.rhat > 2.0).all()
    traj = make().sample(x=x0, n_steps=400, return_trajectory=True, generator=_gen(3))
    want = ChainMoments(*two_pass(traj, 200), 200)
    assert torch.allclose(mom.rhat, want.rhat, rtol=1e-3, atol=0)


# ---------------------------------------------------------------------------------
# validation and edge cases
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps,burn_in", [(3, 0), (2, 0), (5, 2), (4, 5), (4, -1)])
def test_too_few_counted_steps_raise(n_steps, burn_in):
    for s in (ta.UnderdampedLangevin(ta.DoubleWellModel(), step_size=0.05),
              ta.GeneralizedHMC(ta.DoubleWellModel(), step_size=0.1, n_leapfrog_steps=2)):
        with pytest.raises(ValueError):
            s.sample_moments(x=torch.zeros(3, 2), n_steps=n_steps, burn_in=burn_in)


def test_an_odd_count_burns_one_more_step_and_a_wrong_velocity_raises():
    s = ta.UnderdampedLangevin(ta.DoubleWellModel(), step_size=0.05)
    x0 = torch.randn(5, 2, generator=_gen(2))
    xa, a = s.sample_moments(x=x0, n_steps=11, burn_in=2, generator=_gen(4))
    xb, b = s.sample_moments(x=x0, n_steps=11, burn_in=3, generator=_gen(4))
    assert a.half_len == 4 and torch.equal(xa, xb) and torch.equal(a.chain_mean, b.chain_mean)
    assert torch.equal(a.velocity_sq_mean, b.velocity_sq_mean)
    with pytest.raises(ValueError, match="velocity must have the state's shape"):
        s.sample_moments(x=x0, n_steps=8, velocity=torch.zeros(5, 3))


def test_chain_moments_keeps_its_constructor_and_gains_the_velocity_mean():
    mean, m2 = torch.randn(2, 6, 3, generator=_gen(0)), torch.rand(2, 6, 3, generator=_gen(1))
    old = ChainMoments(mean, m2, 5)
    assert old.velocity_sq_mean is None and old.kinetic_temperature is None
    v2 = torch.rand(2, 6, 3, generator=_gen(2))
    v2[1, 4, 0] = float("nan")
    new = ChainMoments(mean, m2, 5, None, None, None, v2)
    others = [i for i in range(6) if i != 4]
    assert new.n_nonfinite == 1
    assert torch.equal(new.kinetic_temperature, v2[:, others].double().mean(dim=(0, 1)))
    assert torch.equal(new.rhat, ChainMoments(mean[:, others], m2[:, others], 5).rhat)


def test_a_nan_chain_is_left_out_and_counted():
    s = ta.UnderdampedLangevin(ta.DoubleWellModel(), step_size=0.05)
    x0 = torch.randn(9, 3, generator=_gen(5))
    bad = x0.clone()
    bad[4, 1] = float("nan")
    _, clean = s.sample_moments(x=x0, n_steps=12, generator=_gen(6))
    _, got = s.sample_moments(x=bad, n_steps=12, generator=_gen(6))
    others = [i for i in range(9) if i != 4]
    assert got.n_nonfinite == 1 and clean.n_nonfinite == 0
    assert torch.equal(got.chain_mean[:, others], clean.chain_mean[:, others])
    assert torch.equal(got.velocity_sq_mean[:, others], clean.velocity_sq_mean[:, others])
    assert torch.isfinite(got.kinetic_temperature).all()


# ---------------------------------------------------------------------------------
# routing: the fused call against the recorder
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["baoab", "ghmc"])
def test_the_fused_route_is_one_call_of_the_entry(fused_cpu, which):  # noqa: F811
    make, rec, _ = fused_cpu
    if which == "baoab":
        s = make(ta.UnderdampedLangevin, step_size=0.05, friction=1.5, temperature=0.8)
    else:
        s = make(ta.GeneralizedHMC, step_size=0.05, n_leapfrog_steps=3, friction=1.5, temperature=0.8)
    x0, v0 = torch.randn(6, 4, generator=_gen(0)), torch.randn(6, 4, generator=_gen(1))
    keep_x, keep_v = x0.clone(), v0.clone()
    x, mom, v = s.sample_moments(x=x0, n_steps=11, burn_in=2, energy=True, velocity=v0, return_velocity=True)
    assert [name for name, _ in rec.calls] == [ENTRY] and dict(_lib.call_counts) == {ENTRY: 1}
    a = rec.calls[0][1]
    assert len(a) == len(_lib._PROTOTYPES[ENTRY][1]) == 27
    assert a[1] == x.data_ptr() and a[2] == v.data_ptr() and a[3:6] == (6, 4, 0 if which == "baoab" else 1)
    assert a[6:9] == (11, 3, 0 if which == "baoab" else 3)  # the odd count burnt one more step
    assert a[9:12] == (0.05, 1.5, 0.8) and a[12] == 0  # velocities were passed: none is drawn
    assert a[13] is not None and a[14] is not None and a[15] is not None
    assert (a[16] is not None) == (which == "baoab")  # v2_mom
    # no trajectory pointer; generalized HMC's acceptance comes from the accept mask, not from the shared counters
    assert a[17:20] == (None, None, None) and (a[20] is not None) == (which == "ghmc") and a[21:24] == (None, None, None)
    assert a[24:26] == (7, 11)
    assert torch.equal(x0, keep_x) and torch.equal(v0, keep_v)
    assert x.data_ptr() != x0.data_ptr() and v.data_ptr() != v0.data_ptr()
    assert mom.half_len == 4 and mom.chain_mean.shape == (2, 6, 4) and mom.energy_mean.shape == (2, 6)
    assert (mom.velocity_sq_mean is not None) == (which == "baoab") and (mom.acceptance_rate is not None) == (which == "ghmc")
    # no velocity: the entry draws it; no energy: no e_mom
    rec.calls.clear()
    s.sample_moments(x=x0, n_steps=8)
    a = rec.calls[0][1]
    assert len(rec.calls) == 1 and a[12] == 1 and a[15] is None and a[6:8] == (8, 0)


def test_a_mask_too_large_falls_to_the_entrys_counters(fused_cpu, monkeypatch):  # noqa: F811
    from torchebm_amd.samplers import kinetic_moments

    make, rec, _ = fused_cpu
    monkeypatch.setattr(kinetic_moments, "MASK_MAX_BYTES", 8 * 6 - 1)
    s = make(ta.GeneralizedHMC, step_size=0.05, n_leapfrog_steps=3)
    _, mom = s.sample_moments(x=torch.zeros(6, 4), n_steps=8)
    a = rec.calls[0][1]
    assert a[20] is None and a[21] is not None and mom.acceptance_rate.shape == (8,)
    assert bool((mom.acceptance_rate == 0).all())  # the recorder launches nothing: the counters keep their zeros


def test_the_reserved_philox_steps_are_samples(fused_cpu, monkeypatch):  # noqa: F811
    from torchebm_amd import _rng

    make, rec, _ = fused_cpu
    asked = []
    monkeypatch.setattr(_rng, "reserve", lambda generator, device, n_steps: asked.append(n_steps) or (7, 11))
    x0 = torch.randn(6, 4, generator=_gen(0))
    make(ta.UnderdampedLangevin, step_size=0.05).sample_moments(x=x0, n_steps=10)
    make(ta.GeneralizedHMC, step_size=0.05, n_leapfrog_steps=2).sample_moments(x=x0, n_steps=10)
    assert asked == [11, 21]


def test_a_failing_launch_raises_and_nothing_falls_back(fused_cpu):  # noqa: F811
    make, rec, _ = fused_cpu
    rec.fail_on = ENTRY
    s = make(ta.UnderdampedLangevin, step_size=0.05)
    with pytest.raises(RuntimeError, match="failed"):
        s.sample_moments(x=torch.zeros(4, 2), n_steps=8)
    assert [name for name, _ in rec.calls] == [ENTRY]


def test_cpu_states_and_other_models_take_the_eager_route():
    before = _lib.call_counts[ENTRY]
    for s in (ta.UnderdampedLangevin(ta.HarmonicModel(k=4.0), step_size=ta.core.schedules.LinearScheduler(0.3, 0.1, 10)),
              ta.GeneralizedHMC(ta.MLPEnergy(3, 64), step_size=0.05, n_leapfrog_steps=2)):
        x, mom = s.sample_moments(x=torch.randn(8, 3, generator=_gen(1)), n_steps=6, generator=_gen(2))
        assert x.shape == (8, 3) and mom.half_len == 3 and torch.isfinite(mom.rhat).all()
    assert _lib.call_counts[ENTRY] == before


# ---------------------------------------------------------------------------------
# the entry's refusals, in front of any launch
# ---------------------------------------------------------------------------------
def _abi_call(desc, *, x=16, v=16, n=4, dim=8, sampler=0, k=8, burn_in=0, L=2, step=0.1, gamma=1.0, temp=1.0, recip=16, mom=16,
              v2_mom=None, v_traj=None):
    _lib.call(ENTRY, desc, x, v, n, dim, sampler, k, burn_in, L, step, gamma, temp, 0, recip, mom, None, v2_mom, None, None, v_traj,
              None, None, None, None, 0, 0, None)


REFUSALS = [
    (dict(dim=257), RuntimeError, r"code -3.*dim 257"),  # EBM_EDIM: one vector per lane
    (dict(dim=0), RuntimeError, r"code -3.*dim 0"),
    (dict(x=None), ValueError, "state pointer is NULL"),
    (dict(v=None), ValueError, "velocity pointer is NULL"),
    (dict(mom=None), ValueError, "recip / mom is NULL"),
    (dict(recip=None), ValueError, "recip / mom is NULL"),
    (dict(sampler=2), ValueError, "sampler=2"),
    (dict(sampler=-1), ValueError, "sampler=-1"),
    (dict(k=7), ValueError, "k_steps=7 burn_in=0"),
    (dict(k=2), ValueError, "k_steps=2 burn_in=0"),
    (dict(k=8, burn_in=6), ValueError, "k_steps=8 burn_in=6"),
    (dict(k=8, burn_in=-2), ValueError, "burn_in=-2"),
    (dict(k=4, burn_in=8), ValueError, "k_steps=4 burn_in=8"),
    (dict(step=0.0), ValueError, "step=0 "),
    (dict(step=-0.1), ValueError, "step=-0.1"),
    (dict(step=float("nan")), ValueError, "step=nan"),
    (dict(step=math.inf), ValueError, "step=inf"),
    (dict(gamma=0.0), ValueError, "gamma=0 "),
    (dict(gamma=float("nan")), ValueError, "gamma=nan"),
    (dict(gamma=math.inf), ValueError, "gamma=inf"),  # BAOAB: finite
    (dict(sampler=1, gamma=float("nan")), ValueError, "gamma=nan"),
    (dict(temp=0.0), ValueError, "temperature=0 "),
    (dict(temp=float("nan")), ValueError, "temperature=nan"),
    (dict(temp=math.inf), ValueError, "temperature=inf"),
    (dict(sampler=1, L=0), ValueError, "n_leapfrog=0"),
    (dict(sampler=1, v2_mom=16), ValueError, "v2_mom / v_traj"),
    (dict(sampler=1, v_traj=16), ValueError, "v2_mom / v_traj"),
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
    with pytest.raises(RuntimeError, match=r"code -2.*no running-moments kernel"):  # EBM_EKIND
        _abi_call(desc)
    desc.kind = _lib.ENERGY_DOUBLE_WELL
    _abi_call(desc, n=0)  # an empty call returns in front of any launch
    _abi_call(desc, n=0, sampler=1, gamma=math.inf)  # ... and an infinite friction is no refusal for generalized HMC
    _abi_call(desc, n=0, L=0)  # ... nor is n_leapfrog for BAOAB, which ignores it
    assert ENTRY in _lib.EXPORTS and ENTRY in _lib._PROTOTYPES and _lib.ABI_VERSION == 9
    assert torch.equal(recip_table(3), torch.tensor([1.0, 0.5, 1.0 / 3.0], dtype=torch.float64).float())


# ---------------------------------------------------------------------------------
# the generalized-HMC cases the GPU tests run
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim,n,k,burn_in,L", GHMC_CASES)
def test_ghmc_cases_meet_the_margin(kind, dim, n, k, burn_in, L):
    c = ghmc_case(kind, dim, n, k, burn_in, L)
    assert c["ref64"]["margin"] > MARGIN_BAR, c["seed"]
    assert torch.equal(c["ref32"]["accepted"], c["ref64"]["accepted"])
    acc = c["ref32"]["accepted"]
    print(kind, dim, "seed", c["seed"], "rejected", int((~acc).sum()), "of", acc.numel())
