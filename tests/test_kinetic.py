"""UnderdampedLangevin without a GPU: the eager route against an independent restatement (kinetic_cases.restate) that replays the
same generator draws, a run cut in two, the law on a quadratic (BAOAB's position marginal is exact there), the sampler's
validation and routing, and the refusals ebm_kinetic_chain_f32 makes in front of any launch."""

import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib
from helpers import hip_calls
from kinetic_cases import constants, energy_spec, law_bar, model_of, oracle_of, restate

ENTRY = "ebm_kinetic_chain_f32"
H, GAMMA, TEMP = 0.05, 1.5, 0.8


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _replay(seed, n, dim, k):
    """The draws the eager route takes from a generator seeded with `seed`: randn(n, dim) for the start velocities, then one per step."""
    g = _gen(seed)
    xi0 = torch.randn(n, dim, generator=g)
    return xi0, torch.stack([torch.randn(n, dim, generator=g) for _ in range(k)])


def _sampler(spec, h=H):
    return ta.UnderdampedLangevin(model_of(spec), step_size=h, friction=GAMMA, temperature=TEMP)


def test_the_constants():
    hh, c1, c2, st = constants(0.3, 2.0, 1.5)
    f32 = lambda v: torch.tensor(v, dtype=torch.float64).float().item()  # noqa: E731
    assert hh == f32(0.15) and c1 == f32(math.exp(-0.6)) and st == f32(math.sqrt(1.5))
    assert c2 == f32(math.sqrt(1.5 * -math.expm1(-1.2))) and abs(c2 * c2 + 1.5 * c1 * c1 - 1.5) < 1e-6  # c2^2 = T (1 - c1^2)
    from torchebm_amd.samplers.kinetic import baoab_constants

    assert list(baoab_constants(0.3, 2.0, 1.5)) == [hh, c1, c2, st]


@pytest.mark.parametrize("kind,dim", [("double_well", 2), ("double_well", 5), ("harmonic", 2), ("harmonic", 5), ("gaussian", 2),
                                      ("gaussian", 5)])
def test_eager_equals_the_restatement_bit_for_bit(kind, dim):
    spec, n, k = energy_spec(kind, dim), 9, 11
    x0 = torch.randn(n, dim, generator=_gen(3))
    xi0, noise = _replay(11, n, dim, k)
    s = _sampler(spec)
    for thin in (1, 3):
        want = restate(oracle_of(spec), x0, None, noise, H, GAMMA, TEMP, thin, torch.float32, xi0=xi0)
        x, v = s.sample(x=x0, n_steps=k, return_velocity=True, generator=_gen(11))
        assert x.shape == (n, dim) and torch.equal(x, want["x"]) and torch.equal(v, want["v"])
        traj = s.sample(x=x0, n_steps=k, thin=thin, return_trajectory=True, generator=_gen(11))
        assert traj.shape == (n, k // thin, dim) and torch.equal(traj, want["traj"])
    assert not torch.equal(want["x"], x0)
    # a given start velocity is used as it is
    v0 = torch.randn(n, dim, generator=_gen(4))
    want = restate(oracle_of(spec), x0, v0, noise, H, GAMMA, TEMP, 1, torch.float32)
    g = _gen(11)
    torch.randn(n, dim, generator=g)  # (the draw the start velocities would have taken)
    keep_x, keep_v = x0.clone(), v0.clone()
    x, v = s.sample(x=x0, n_steps=k, velocity=v0, return_velocity=True, generator=g)
    assert torch.equal(x, want["x"]) and torch.equal(v, want["v"])
    assert torch.equal(x0, keep_x) and torch.equal(v0, keep_v), "the caller's tensors were touched"


@pytest.mark.parametrize("kind", ["double_well", "gaussian"])
def test_a_run_cut_in_two_is_the_uncut_run(kind):
    spec, n, dim, k1, k2 = energy_spec(kind, 5), 9, 5, 4, 7
    x0 = torch.randn(n, dim, generator=_gen(5))
    s = _sampler(spec)
    whole_x, whole_v = s.sample(x=x0, n_steps=k1 + k2, return_velocity=True, generator=_gen(12))
    g = _gen(12)
    x, v = s.sample(x=x0, n_steps=k1, return_velocity=True, generator=g)
    x, v = s.sample(x=x, n_steps=k2, velocity=v, return_velocity=True, reset_schedulers=False, generator=g)
    assert torch.equal(x, whole_x) and torch.equal(v, whole_v)


def check_harmonic_law(x, v, diag, k_spring, temp, h):
    """var(x) k / T = 1 and var(v) / T = 1 - h^2 k / 4 over all final coordinates, each within 4.5 standard errors of the
    variance of N independent normal values; the diagnostics' kinetic temperature is that var(v)."""
    bar = law_bar(x.numel())
    var_x, var_v = x.double().var().item(), v.double().var().item()
    want_v = temp * (1.0 - h * h * k_spring / 4.0)
    print(f"var(x) k / T = {var_x * k_spring / temp:.4f} (1), var(v) = {var_v:.4f} ({want_v:.4f}), bar {bar:.4f}, "
          f"kinetic_temperature = {diag['kinetic_temperature'].item():.4f}")
    assert abs(var_x * k_spring / temp - 1.0) < bar
    assert abs(var_v / want_v - 1.0) < bar
    assert abs(diag["kinetic_temperature"].item() - var_v) < 1e-3  # (the mean of v^2 against the centred variance)


LAW_SEED = 0


def law_start(n, dim, k_spring, temp, seed, device=None):
    x0 = math.sqrt(temp / k_spring) * torch.randn(n, dim, generator=_gen(seed))
    return x0 if device is None else x0.to(device)


def test_the_position_marginal_of_a_harmonic_well_is_exact():
    """h = 0.3 on k = 4: Euler-Maruyama at the matching step h^2 / 2 is off by 1.099 here; BAOAB by nothing, and var(v) = 0.91."""
    n, dim = 4096, 4
    s = ta.UnderdampedLangevin(ta.HarmonicModel(k=4.0), step_size=0.3, friction=1.0, temperature=1.0)
    (x, diag, v) = s.sample(x=law_start(n, dim, 4.0, 1.0, LAW_SEED), n_steps=400, return_diagnostics=True, return_velocity=True,
                            generator=_gen(LAW_SEED))
    assert math.isclose(law_bar(n * dim), 0.0497, abs_tol=1e-4)
    check_harmonic_law(x, v, diag, 4.0, 1.0, 0.3)


def test_a_second_temperature():
    n, dim = 4096, 4
    s = ta.UnderdampedLangevin(ta.HarmonicModel(k=1.0), step_size=1.0, friction=0.5, temperature=2.0)
    (x, diag, v) = s.sample(x=law_start(n, dim, 1.0, 2.0, LAW_SEED), n_steps=200, return_diagnostics=True, return_velocity=True,
                            generator=_gen(LAW_SEED))
    check_harmonic_law(x, v, diag, 1.0, 2.0, 1.0)


def test_diagnostics_of_the_eager_route():
    spec, n, dim, k = energy_spec("double_well", 4), 128, 4, 12
    x0 = torch.randn(n, dim, generator=_gen(5))
    xi0, noise = _replay(13, n, dim, k)
    want = restate(oracle_of(spec), x0, None, noise, H, GAMMA, TEMP, 3, torch.float32, xi0=xi0)
    out, diag, v = _sampler(spec).sample(x=x0, n_steps=k, thin=3, return_trajectory=True, return_diagnostics=True, return_velocity=True,
                                         generator=_gen(13))
    assert torch.equal(out, want["traj"]) and out.shape == (n, 4, dim) and torch.equal(v, want["v"])
    assert diag["mean"].shape == diag["var"].shape == (4, dim) and diag["energy"].shape == (4,)
    assert torch.allclose(diag["mean"], want["traj"].mean(dim=0), atol=1e-6)
    assert torch.allclose(diag["var"], want["traj"].var(dim=0, unbiased=False).clamp(1e-10, 1e10), atol=1e-6)
    e = torch.stack([oracle_of(spec).energy(want["traj"][:, j]).mean() for j in range(4)])
    assert torch.allclose(diag["energy"], e, rtol=1e-5)
    assert torch.allclose(diag["kinetic_temperature"], want["v"].square().mean(), rtol=1e-6)


def test_validation():
    m = ta.DoubleWellModel()
    for kw in (dict(friction=0.0), dict(friction=-1.0), dict(temperature=0.0), dict(temperature=-2.0), dict(step_size=0.0),
               dict(step_size=-0.1)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            ta.UnderdampedLangevin(m, **kw)
    s = ta.UnderdampedLangevin(m)
    with pytest.raises(ValueError, match="thin"):
        s.sample(dim=2, thin=0)
    with pytest.raises(ValueError, match="dim must be provided"):
        s.sample()
    with pytest.raises(ValueError, match="velocity must have the state's shape"):
        s.sample(x=torch.zeros(3, 2), velocity=torch.zeros(3, 3))
    assert ta.samplers.UnderdampedLangevin is ta.UnderdampedLangevin
    # x = None draws the start; no step returns the start and its drawn velocities
    out = s.sample(dim=3, n_samples=5, n_steps=3, generator=_gen(1))
    assert out.shape == (5, 3) and torch.isfinite(out).all()
    x0 = torch.ones(4, 2)
    x, v = s.sample(x=x0, n_steps=0, return_velocity=True, generator=_gen(1))
    assert torch.equal(x, x0) and x.data_ptr() != x0.data_ptr() and torch.equal(v, torch.randn(4, 2, generator=_gen(1)))


def test_routing():
    """Only a CUDA fp32 state on an analytic energy with a constant step size and dim <= 256 is fused; a scheduler on step_size,
    an nn.Module energy and the CPU take the eager route and never reach the entry."""
    cpu = torch.zeros(3, 2)
    s = ta.UnderdampedLangevin(ta.DoubleWellModel(), step_size=0.05)
    assert s._route(cpu) == ("eager", None)
    sched = ta.UnderdampedLangevin(ta.HarmonicModel(k=4.0), step_size=ta.core.schedules.LinearScheduler(0.3, 0.1, 10))
    assert not sched.schedulers["step_size"].is_constant() and sched._route(cpu)[0] == "eager"

    class AsCuda:  # what _route reads of a state, with no GPU at hand
        def __init__(self, dim, dtype=torch.float32, ndim=2):
            self.is_cuda, self.dtype, self.ndim, self.shape, self.device = True, dtype, ndim, (8, dim), torch.device("cpu")

    assert s._route(AsCuda(256))[0] == "fused" and s._route(AsCuda(2))[0] == "fused"
    assert s._route(AsCuda(257))[0] == "eager" and s._route(AsCuda(8, torch.float64))[0] == "eager" and s._route(AsCuda(8, ndim=3))[0] == "eager"
    assert sched._route(AsCuda(8))[0] == "eager"

    class Quartic(ta.BaseModel):
        def forward(self, x):
            return (x**4).sum(dim=-1)

    assert ta.UnderdampedLangevin(Quartic(), step_size=0.01)._route(AsCuda(8))[0] == "eager"
    assert ta.UnderdampedLangevin(ta.MLPEnergy(8, 64), step_size=0.01)._route(AsCuda(8))[0] == "eager"
    before = hip_calls(ENTRY)
    # the scheduled step size is read before every step: k = 1 with h decaying from 0.3 stays a harmonic well's law
    g = _gen(2)
    x, v = sched.sample(x=0.5 * torch.randn(2048, 2, generator=g), n_steps=30, return_velocity=True, generator=g)
    assert abs(x.var().item() * 4.0 - 1.0) < 0.15
    out = ta.UnderdampedLangevin(Quartic(), step_size=0.01).sample(dim=3, n_samples=16, n_steps=6, generator=_gen(2))
    assert out.shape == (16, 3) and torch.isfinite(out).all()
    assert hip_calls(ENTRY) == before


def _abi_call(desc, *, x=16, v=16, n=4, dim=8, k=3, h=0.1, gamma=1.0, temp=1.0, thin=1):
    _lib.call(ENTRY, desc, x, v, n, dim, k, h, gamma, temp, 0, thin, None, None, 0, 0, None)


REFUSALS = [
    (dict(dim=257), RuntimeError, r"code -3.*dim 257"),  # EBM_EDIM: one vector per lane
    (dict(k=0), ValueError, "k_steps=0"),
    (dict(thin=0), ValueError, "thin=0"),
    (dict(x=None), ValueError, "state pointer is NULL"),
    (dict(v=None), ValueError, "velocity pointer is NULL"),
    (dict(h=0.0), ValueError, "h=0 "),
    (dict(h=-0.1), ValueError, "h=-0.1"),
    (dict(gamma=0.0), ValueError, "gamma=0 "),
    (dict(temp=0.0), ValueError, "temperature=0 "),
    (dict(temp=float("nan")), ValueError, "temperature=nan"),
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
    with pytest.raises(RuntimeError, match=r"code -2.*no underdamped-Langevin kernel"):  # EBM_EKIND
        _abi_call(desc)
    desc.kind = _lib.ENERGY_DOUBLE_WELL
    _abi_call(desc, n=0)  # an empty call returns in front of any launch
    assert ENTRY in _lib.EXPORTS and _lib.ABI_VERSION == 9
