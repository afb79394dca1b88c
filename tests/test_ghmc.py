"""GeneralizedHMC without a GPU: the eager route against an independent restatement (ghmc_cases.restate) that replays the same
generator draws, a run cut in two, friction = inf against HamiltonianMonteCarlo, the decisions of every GPU case, the law on a
quadratic (exact for every step size), the sampler's validation and routing, the one recorded launch of the fused route, and
the refusals ebm_ghmc_chain_f32 makes in front of any launch."""

import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import fused_cpu, hip_calls  # noqa: F401  (fused_cpu: the fixture)
from ghmc_cases import (ALL_CASES, CASES, LAW_SEED, LAW_SHAPE, LAW_STEPS, LAWS, MARGIN_BAR, case, constants, energy_spec, law_bar,
                        model_of, oracle_of, restate, step_size)

ENTRY = "ebm_ghmc_chain_f32"
GAMMA, TEMP = 1.5, 0.8


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _replay(seed, n, dim, n_mh, with_v0=True):
    """The draws the eager route takes from a generator seeded with `seed`: randn(n, dim) for the start velocities (only when
    none are passed), then randn(n, dim) and rand(n) per transition."""
    g = _gen(seed)
    xi0 = torch.randn(n, dim, generator=g) if with_v0 else None
    z, u = [], []
    for _ in range(n_mh):
        z.append(torch.randn(n, dim, generator=g))
        u.append(torch.rand(n, generator=g))
    return xi0, torch.stack(z), torch.stack(u)


def _sampler(spec, eps, L, gamma=GAMMA, temp=TEMP):
    return ta.GeneralizedHMC(model_of(spec), step_size=eps, n_leapfrog_steps=L, friction=gamma, temperature=temp)


def test_the_constants():
    c1, c2, st, beta = constants(0.1, 3, 2.0, 1.5)
    f32 = lambda v: torch.tensor(v, dtype=torch.float64).float().item()  # noqa: E731
    assert c1 == f32(math.exp(-0.6)) and st == f32(math.sqrt(1.5)) and beta == f32(1.0 / 1.5)
    assert c2 == f32(math.sqrt(1.5 * -math.expm1(-1.2))) and abs(c2 * c2 + 1.5 * c1 * c1 - 1.5) < 1e-6  # c2^2 = T (1 - c1^2)
    from torchebm_amd.samplers.ghmc import ghmc_constants

    assert list(ghmc_constants(0.1, 3, 2.0, 1.5)) == [c1, c2, st, beta]
    assert list(ghmc_constants(0.1, 3, math.inf, 1.5)) == constants(0.1, 3, math.inf, 1.5) == [0.0, st, st, beta]


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("kind,dim", [("double_well", 2), ("double_well", 5), ("harmonic", 2), ("harmonic", 5), ("gaussian", 2),
                                      ("gaussian", 5)])
def test_eager_equals_the_restatement_bit_for_bit(kind, dim, L):
    # (twice the step size of the GPU cases: these 99 decisions then reject up to a fifth of their proposals, so the flip is in them)
    spec, n, n_mh, eps = energy_spec(kind, dim), 9, 11, 2.0 * step_size(kind, dim)
    x0 = torch.randn(n, dim, generator=_gen(3))
    xi0, z, u = _replay(11, n, dim, n_mh)
    s = _sampler(spec, eps, L)
    for thin in (1, 3):
        want = restate(oracle_of(spec), x0, None, z, u, eps, L, GAMMA, TEMP, torch.float32, thin, xi0=xi0)
        x, v = s.sample(x=x0, n_steps=n_mh, return_velocity=True, generator=_gen(11))
        assert x.shape == (n, dim) and torch.equal(x, want["x"]) and torch.equal(v, want["v"])
        traj, diag = s.sample(x=x0, n_steps=n_mh, thin=thin, return_trajectory=True, return_diagnostics=True, generator=_gen(11))
        assert traj.shape == (n, n_mh // thin, dim) and torch.equal(traj, want["traj"])
        # the accept mask, through the acceptance rate of every kept transition
        assert torch.equal(diag["acceptance_rate"], want["accepted"][thin - 1 :: thin][: n_mh // thin].float().mean(dim=1))
    assert not torch.equal(want["x"], x0)
    # a given start velocity is used as it is
    v0 = torch.randn(n, dim, generator=_gen(4))
    _, z, u = _replay(11, n, dim, n_mh, with_v0=False)
    want = restate(oracle_of(spec), x0, v0, z, u, eps, L, GAMMA, TEMP, torch.float32)
    keep_x, keep_v = x0.clone(), v0.clone()
    x, v = s.sample(x=x0, n_steps=n_mh, velocity=v0, return_velocity=True, generator=_gen(11))
    assert torch.equal(x, want["x"]) and torch.equal(v, want["v"])
    assert torch.equal(x0, keep_x) and torch.equal(v0, keep_v), "the caller's tensors were touched"


def test_the_eager_cases_accept_and_reject():
    """The runs above take both decisions, so the flip is in them."""
    seen = torch.zeros(2, dtype=torch.bool)
    for kind, dim in (("double_well", 5), ("harmonic", 5), ("gaussian", 5)):
        spec, eps = energy_spec(kind, dim), 2.0 * step_size(kind, dim)
        xi0, z, u = _replay(11, 9, dim, 11)
        acc = restate(oracle_of(spec), torch.randn(9, dim, generator=_gen(3)), None, z, u, eps, 3, GAMMA, TEMP, xi0=xi0)["accepted"]
        seen |= torch.tensor([bool(acc.any()), bool((~acc).any())])
    assert seen.all()


@pytest.mark.parametrize("kind", ["double_well", "gaussian"])
def test_a_run_cut_in_two_is_the_uncut_run(kind):
    spec, n, dim, k1, k2 = energy_spec(kind, 5), 9, 5, 4, 7
    x0 = torch.randn(n, dim, generator=_gen(5))
    s = _sampler(spec, 2.0 * step_size(kind, dim), 3)
    whole_x, whole_v = s.sample(x=x0, n_steps=k1 + k2, return_velocity=True, generator=_gen(12))
    g = _gen(12)
    x, v = s.sample(x=x0, n_steps=k1, return_velocity=True, generator=g)
    x, v = s.sample(x=x, n_steps=k2, velocity=v, return_velocity=True, reset_schedulers=False, generator=g)
    assert torch.equal(x, whole_x) and torch.equal(v, whole_v)


@pytest.mark.parametrize("kind", ["double_well", "gaussian"])
def test_infinite_friction_is_hamiltonian_monte_carlo(kind):
    """friction = inf, T = 1: c1 = 0 and c2 = 1, every transition draws a fresh velocity.  With a start velocity passed the draw
    orders coincide -- randn(n, dim) then rand(n) per transition, HamiltonianMonteCarlo's own -- and the runs are equal bit for
    bit; without one this sampler draws its start velocities first (which the refresh then discards), one field ahead of HMC."""
    spec, n, dim, n_mh, L = energy_spec(kind, 5), 9, 5, 11, 3
    eps = 2.0 * step_size(kind, dim)
    x0 = torch.randn(n, dim, generator=_gen(6))
    hmc = ta.HamiltonianMonteCarlo(model_of(spec), step_size=eps, n_leapfrog_steps=L)
    want, want_diag = hmc.sample(x=x0, n_steps=n_mh, return_diagnostics=True, generator=_gen(13))
    s = _sampler(spec, eps, L, gamma=math.inf, temp=1.0)
    got, diag = s.sample(x=x0, n_steps=n_mh, velocity=torch.zeros(n, dim), return_diagnostics=True, generator=_gen(13))
    assert torch.equal(got, want) and torch.equal(diag["acceptance_rate"], want_diag["acceptance_rate"])
    assert 0.0 < diag["acceptance_rate"].mean() < 1.0 or not torch.equal(got, x0)
    # the other order, against the restatement
    xi0, z, u = _replay(13, n, dim, n_mh)
    ref = restate(oracle_of(spec), x0, None, z, u, eps, L, math.inf, 1.0, xi0=xi0)
    assert torch.equal(s.sample(x=x0, n_steps=n_mh, generator=_gen(13)), ref["x"])


@pytest.mark.parametrize("kind,dim,n,n_mh,thin,L", ALL_CASES)
def test_no_gpu_case_is_borderline(kind, dim, n, n_mh, thin, L):
    """Every case test_ghmc_gpu.py runs: the fp64 restatement decides nothing closer than MARGIN_BAR to its threshold, and the
    fp32 restatement takes the same decisions."""
    c = case(kind, dim, n, n_mh, thin, L)
    assert c["ref64"]["margin"] > MARGIN_BAR, (c["seed"], c["ref64"]["margin"])
    assert torch.equal(c["ref32"]["accepted"], c["ref64"]["accepted"])
    assert c["ref32"]["accepted"].shape == (n_mh, n) and c["ref32"]["traj"].shape == (n, n_mh // thin, dim)


@pytest.mark.parametrize("kind", list(CASES))
def test_every_group_accepts_and_rejects(kind):
    acc = torch.cat([case(*c)["ref32"]["accepted"].flatten() for c in CASES[kind]])
    print(kind, "rejected", int((~acc).sum()), "of", acc.numel())
    assert acc.any() and (~acc).any()


def law_start(n, dim, k_spring, temp, seed, device=None):
    x0 = math.sqrt(temp / k_spring) * torch.randn(n, dim, generator=_gen(seed))
    return x0 if device is None else x0.to(device)


def check_harmonic_law(x, v, diag, k_spring, temp):
    """var(x) k / T = 1 and var(v) / T = 1 over all final coordinates, each within 4.5 standard errors of the variance of N
    independent normal values; the diagnostics' kinetic temperature is that var(v)."""
    bar = law_bar(x.numel())
    var_x, var_v = x.double().var().item(), v.double().var().item()
    print(f"var(x) k / T = {var_x * k_spring / temp:.4f}, var(v) / T = {var_v / temp:.4f}, bar {bar:.4f}, "
          f"acceptance = {diag['acceptance_rate'].mean().item():.3f}, kinetic_temperature = {diag['kinetic_temperature'].item():.4f}")
    assert abs(var_x * k_spring / temp - 1.0) < bar
    assert abs(var_v / temp - 1.0) < bar
    assert abs(diag["kinetic_temperature"].item() - var_v) < 2e-3 * temp  # (the mean of v^2 against the centred variance)
    assert 0.5 < diag["acceptance_rate"].mean().item() < 1.0


@pytest.mark.parametrize("k_spring,eps,gamma,temp,L", LAWS)
def test_the_law_of_a_harmonic_well_is_exact(k_spring, eps, gamma, temp, L):
    """h = 0.3 on k = 4 leaves BAOAB's var(v) at 0.909 T; the adjusted chain has var(x) k = var(v) = T at every step size."""
    n, dim = LAW_SHAPE
    assert math.isclose(law_bar(n * dim), 0.0497, abs_tol=1e-4)
    s = ta.GeneralizedHMC(ta.HarmonicModel(k=k_spring), step_size=eps, n_leapfrog_steps=L, friction=gamma, temperature=temp)
    x, diag, v = s.sample(x=law_start(n, dim, k_spring, temp, LAW_SEED), n_steps=LAW_STEPS, thin=LAW_STEPS // 4, return_diagnostics=True,
                          return_velocity=True, generator=_gen(LAW_SEED))
    check_harmonic_law(x, v, diag, k_spring, temp)


def test_diagnostics_of_the_eager_route():
    spec, n, dim, n_mh, L = energy_spec("double_well", 4), 128, 4, 12, 2
    eps = 2.0 * step_size("double_well", dim)
    x0 = torch.randn(n, dim, generator=_gen(5))
    xi0, z, u = _replay(13, n, dim, n_mh)
    want = restate(oracle_of(spec), x0, None, z, u, eps, L, GAMMA, TEMP, torch.float32, 3, xi0=xi0)
    out, diag, v = _sampler(spec, eps, L).sample(x=x0, n_steps=n_mh, thin=3, return_trajectory=True, return_diagnostics=True,
                                                 return_velocity=True, generator=_gen(13))
    assert torch.equal(out, want["traj"]) and out.shape == (n, 4, dim) and torch.equal(v, want["v"])
    assert diag["mean"].shape == diag["var"].shape == (4, dim) and diag["energy"].shape == diag["acceptance_rate"].shape == (4,)
    assert torch.allclose(diag["mean"], want["traj"].mean(dim=0), atol=1e-6)
    assert torch.allclose(diag["var"], want["traj"].var(dim=0, unbiased=False).clamp(1e-10, 1e10), atol=1e-6)
    e = torch.stack([oracle_of(spec).energy(want["traj"][:, j]).mean() for j in range(4)])
    assert torch.allclose(diag["energy"], e, rtol=1e-5)
    assert torch.equal(diag["acceptance_rate"], want["accepted"][2::3].float().mean(dim=1))
    assert torch.allclose(diag["kinetic_temperature"], want["v"].square().mean(), rtol=1e-6)


def test_validation():
    m = ta.DoubleWellModel()
    for kw in (dict(friction=0.0), dict(friction=-1.0), dict(friction=float("nan")), dict(temperature=0.0), dict(temperature=-2.0),
               dict(temperature=math.inf), dict(step_size=0.0), dict(step_size=-0.1), dict(n_leapfrog_steps=0), dict(n_leapfrog_steps=1.5)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            ta.GeneralizedHMC(m, **kw)
    assert ta.GeneralizedHMC(m, friction=math.inf).friction == math.inf
    s = ta.GeneralizedHMC(m)
    with pytest.raises(ValueError, match="thin"):
        s.sample(dim=2, thin=0)
    with pytest.raises(ValueError, match="dim must be provided"):
        s.sample()
    with pytest.raises(ValueError, match="velocity must have the state's shape"):
        s.sample(x=torch.zeros(3, 2), velocity=torch.zeros(3, 3))
    from torchebm_amd.samplers import GeneralizedHMC

    assert GeneralizedHMC is ta.GeneralizedHMC is ta.samplers.GeneralizedHMC and "GeneralizedHMC" in ta.samplers.__all__
    # x = None draws the start; no transition returns the start and its drawn velocities
    out = s.sample(dim=3, n_samples=5, n_steps=3, generator=_gen(1))
    assert out.shape == (5, 3) and torch.isfinite(out).all()
    x0 = torch.ones(4, 2)
    x, v = s.sample(x=x0, n_steps=0, return_velocity=True, generator=_gen(1))
    assert torch.equal(x, x0) and x.data_ptr() != x0.data_ptr() and torch.equal(v, torch.randn(4, 2, generator=_gen(1)))


def test_routing():
    """Only a CUDA fp32 2-D state on an analytic energy with a constant step size and dim <= 256 is fused; a scheduler on
    step_size, an nn.Module energy and the CPU take the eager route and never reach the entry."""
    cpu = torch.zeros(3, 2)
    s = ta.GeneralizedHMC(ta.DoubleWellModel(), step_size=0.05)
    assert s._route(cpu) == ("eager", None)
    sched = ta.GeneralizedHMC(ta.HarmonicModel(k=4.0), step_size=ta.core.schedules.LinearScheduler(0.3, 0.1, 10), n_leapfrog_steps=2)
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

    assert ta.GeneralizedHMC(Quartic(), step_size=0.01)._route(AsCuda(8))[0] == "eager"
    assert ta.GeneralizedHMC(ta.MLPEnergy(8, 64), step_size=0.01)._route(AsCuda(8))[0] == "eager"
    before = hip_calls(ENTRY)
    # the scheduled step size is read before every transition: the law of the harmonic well holds whatever the schedule
    g = _gen(2)
    x, v = sched.sample(x=0.5 * torch.randn(2048, 2, generator=g), n_steps=30, return_velocity=True, generator=g)
    assert abs(x.var().item() * 4.0 - 1.0) < 0.15 and abs(v.var().item() - 1.0) < 0.15
    out = ta.GeneralizedHMC(Quartic(), step_size=0.05, n_leapfrog_steps=2).sample(dim=3, n_samples=16, n_steps=6, generator=_gen(2))
    assert out.shape == (16, 3) and torch.isfinite(out).all()
    assert hip_calls(ENTRY) == before


def test_the_fused_route_is_one_recorded_launch(fused_cpu, monkeypatch):  # noqa: F811
    make, rec, _ = fused_cpu
    reserved = []
    monkeypatch.setattr(_rng, "reserve", lambda generator, device, n_steps: reserved.append(n_steps) or (7, 11))
    s = make(ta.GeneralizedHMC, step_size=0.05, n_leapfrog_steps=3, friction=1.5, temperature=0.8)
    x0 = torch.randn(16, 4, generator=_gen(1))
    keep = x0.clone()
    x, v = s.sample(x=x0, n_steps=5, return_velocity=True)
    assert reserved == [2 * 5 + 1]
    assert [name for name, _ in rec.calls] == [ENTRY]
    args = rec.calls[0][1]
    assert args[1] == x.data_ptr() != x0.data_ptr() and args[2] == v.data_ptr() and torch.equal(x0, keep)
    assert tuple(args[3:]) == (16, 4, 5, 3, 0.05, 1.5, 0.8, 1, 1, None, None, None, None, 7, 11, None)
    # a passed velocity is copied and read (draw_v0 = 0); trajectory and diagnostics ask for the kept states and the mask
    rec.calls.clear()
    v0 = torch.ones(16, 4)
    traj, diag, v = s.sample(x=x0, n_steps=5, thin=2, velocity=v0, return_trajectory=True, return_diagnostics=True, return_velocity=True)
    name, args = rec.calls[0]
    assert name == ENTRY and reserved == [11, 11] and args[2] == v.data_ptr() != v0.data_ptr() and torch.equal(v0, torch.ones(16, 4))
    assert tuple(args[3:13]) == (16, 4, 5, 3, 0.05, 1.5, 0.8, 0, 2, traj.data_ptr()) and args[13] is not None and args[14:16] == (None, None)
    assert traj.shape == (16, 2, 4) and diag["acceptance_rate"].shape == (2,) and len(rec.named(ENTRY)) == 1


def _abi_call(desc, *, x=16, v=16, n=4, dim=8, n_mh=3, L=2, eps=0.1, gamma=1.0, temp=1.0, thin=1):
    _lib.call(ENTRY, desc, x, v, n, dim, n_mh, L, eps, gamma, temp, 0, thin, None, None, None, None, 0, 0, None)


REFUSALS = [
    (dict(dim=257), RuntimeError, r"code -3.*dim 257"),  # EBM_EDIM: one vector per lane
    (dict(dim=0), RuntimeError, r"code -3.*dim 0"),
    (dict(n_mh=0), ValueError, "n_mh=0"),
    (dict(L=0), ValueError, "n_leapfrog=0"),
    (dict(thin=0), ValueError, "thin=0"),
    (dict(x=None), ValueError, "state pointer is NULL"),
    (dict(v=None), ValueError, "velocity pointer is NULL"),
    (dict(eps=0.0), ValueError, "eps=0 "),
    (dict(eps=-0.1), ValueError, "eps=-0.1"),
    (dict(eps=float("nan")), ValueError, "eps=nan"),
    (dict(gamma=0.0), ValueError, "gamma=0 "),
    (dict(gamma=float("nan")), ValueError, "gamma=nan"),
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
    with pytest.raises(RuntimeError, match=r"code -2.*no generalized-HMC kernel"):  # EBM_EKIND
        _abi_call(desc)
    desc.kind = _lib.ENERGY_DOUBLE_WELL
    _abi_call(desc, n=0)  # an empty call returns in front of any launch
    _abi_call(desc, n=0, gamma=math.inf)  # ... and an infinite friction is no refusal
    assert ENTRY in _lib.EXPORTS and ENTRY in _lib._PROTOTYPES and _lib.ABI_VERSION == 9
