"""Dual-averaging step-size adaptation without a GPU: the cases of adapt_cases.py, the eager route of adapt_step_size on both
samplers against the independent restatement on the torch generator's draws, a run cut in two, the table builder, the pooling,
`apply`, validation and routing, the one recorded launch of the fused route, and the refusals ebm_ghmc_adapt_chain_f32 makes in
front of any launch."""

import math
import os
import re

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from torchebm_amd.samplers import adapt
from helpers import fused_cpu, hip_calls  # noqa: F401  (fused_cpu: the fixture)
import adapt_cases as ac
from adapt_cases import ALL_CASES, CASES, GAMMA, MARGIN_BAR, TEMP, case, energy_spec, model_of, oracle_of, restate, step_size

ENTRY = "ebm_ghmc_adapt_chain_f32"
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _replay(seed, n, dim, n_mh, with_v0=True):
    """The draws the eager route takes: randn(n, dim) for the start velocities (only when none are passed), then randn(n, dim)
    and rand(n) per transition."""
    g = _gen(seed)
    xi0 = torch.randn(n, dim, generator=g) if with_v0 else None
    z, u = [], []
    for _ in range(n_mh):
        z.append(torch.randn(n, dim, generator=g))
        u.append(torch.rand(n, generator=g))
    return xi0, torch.stack(z), torch.stack(u)


# ---------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim,n,n_mh,thin,L", ALL_CASES)
def test_every_case_finds_its_seed(kind, dim, n, n_mh, thin, L):
    c = case(kind, dim, n, n_mh, thin, L)
    assert c["found"], "no seed among 200"
    assert c["ref64"]["margin"] > MARGIN_BAR, (c["seed"], c["ref64"]["margin"])
    assert torch.equal(c["ref32"]["accepted"], c["ref64"]["accepted"])
    assert c["ref32"]["accepted"].shape == c["ref32"]["eps_trace"].shape == (n_mh, n) and c["ref32"]["da"].shape == (3, n)
    trace = c["ref32"]["eps_trace"] / c["eps0"]
    assert torch.equal(trace[0], torch.full((n,), ac.f32(c["eps0"])) / c["eps0"])
    if n_mh >= 4:  # the controller moved some chain's step size out of [0.5, 2] eps0
        assert bool(((trace < 0.5) | (trace > 2.0)).any())
    assert n_mh in (2, 4, 6)


@pytest.mark.parametrize("kind", list(CASES))
def test_every_group_accepts_and_rejects(kind):
    acc = torch.cat([case(*c)["ref32"]["accepted"].flatten() for c in CASES[kind]])
    assert acc.any() and (~acc).any()


def test_the_table_is_the_formula_in_double():
    for m0, t0, g, kappa in ((0, 10.0, 0.05, 0.75), (7, 3.0, 0.1, 0.6)):
        got = adapt.da_table(9, m0, t0, g, kappa)
        assert got.dtype == torch.float32 and got.shape == (9, 5)
        for t in range(9):
            m = float(m0 + t + 1)
            w, k = 1.0 / (m + t0), m ** (-kappa)
            want = [ac.f32(1.0 - w), ac.f32(w), ac.f32(math.sqrt(m) / g), ac.f32(k), ac.f32(1.0 - k)]
            assert got[t, :3].tolist() == want[:3]
            assert got[t, 3:].tolist() == pytest.approx(want[3:], rel=1.2e-7, abs=0)  # (pow in torch against pow in libm: an fp32 ulp at most)
    assert adapt.da_table(0).shape == (0, 5)


def test_the_pooling():
    eps = torch.tensor([0.1, 0.2, 0.4, float("nan"), float("inf"), 0.0, 0.8, 100.0])
    pooled = adapt.pool_step_sizes(eps)
    assert pooled.ndim == 0 and math.isclose(pooled.item(), 0.4, rel_tol=1e-6)  # the median of the five finite logs
    assert math.isnan(adapt.pool_step_sizes(torch.tensor([float("nan")])).item())


# ---------------------------------------------------------------------------------
# the eager route
# ---------------------------------------------------------------------------------
def _samplers(spec, eps, L):
    return {"ghmc": (ta.GeneralizedHMC(model_of(spec), step_size=eps, n_leapfrog_steps=L, friction=GAMMA, temperature=TEMP), GAMMA, TEMP),
            "hmc": (ta.HamiltonianMonteCarlo(model_of(spec), step_size=eps, n_leapfrog_steps=L), math.inf, 1.0)}


@pytest.mark.parametrize("which", ["ghmc", "hmc"])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("kind,dim", [("double_well", 2), ("double_well", 5), ("harmonic", 2), ("harmonic", 5), ("gaussian", 2),
                                      ("gaussian", 5)])
def test_eager_equals_the_restatement_bit_for_bit(kind, dim, L, which):
    spec, n, n_mh, eps = energy_spec(kind, dim), 9, 11, 2.0 * step_size(kind, dim)
    x0 = torch.randn(n, dim, generator=_gen(3))
    xi0, z, u = _replay(11, n, dim, n_mh)
    s, gamma, temp = _samplers(spec, eps, L)[which]
    want = restate(oracle_of(spec), x0, None, z, u, eps, L, gamma, temp, torch.float32, xi0=xi0)
    keep = x0.clone()
    r = s.adapt_step_size(x=x0, n_steps=n_mh, generator=_gen(11), apply=False)
    assert torch.equal(r.x, want["x"]) and torch.equal(r.velocity, want["v"]) and torch.equal(x0, keep)
    assert torch.equal(r.da, want["da"]) and torch.equal(r.step_sizes, want["da"][0]) and torch.equal(r.acceptance, want["alpha_mean"])
    assert r.step_size.ndim == 0 and torch.equal(r.step_size, want["da"][0].log().median().exp())
    assert s.get_scheduled_value("step_size") == eps  # apply=False
    assert not torch.equal(want["da"][0], torch.full((n,), ac.f32(eps))) and want["accepted"].any()
    # a given start velocity is used as it is, and another start step size moves mu with it
    v0 = torch.randn(n, dim, generator=_gen(4))
    _, z, u = _replay(11, n, dim, n_mh, with_v0=False)
    want = restate(oracle_of(spec), x0, v0, z, u, 0.5 * eps, L, gamma, temp, torch.float32, delta=0.65)
    r = s.adapt_step_size(x=x0, n_steps=n_mh, velocity=v0, init_step_size=0.5 * eps, target_accept=0.65, generator=_gen(11), apply=False)
    assert torch.equal(r.x, want["x"]) and torch.equal(r.velocity, want["v"]) and torch.equal(r.da, want["da"])


def test_the_eager_cases_accept_and_reject():
    seen = torch.zeros(2, dtype=torch.bool)
    for kind, dim in (("double_well", 5), ("harmonic", 5), ("gaussian", 5)):
        spec, eps = energy_spec(kind, dim), 2.0 * step_size(kind, dim)
        xi0, z, u = _replay(11, 9, dim, 11)
        acc = restate(oracle_of(spec), torch.randn(9, dim, generator=_gen(3)), None, z, u, eps, 3, GAMMA, TEMP, xi0=xi0)["accepted"]
        seen |= torch.tensor([bool(acc.any()), bool((~acc).any())])
    assert seen.all()


@pytest.mark.parametrize("kind", ["double_well", "gaussian"])
def test_a_run_cut_in_two_is_the_uncut_run(kind):
    """An open first part (the last iterate kept) continued with the table at m0 = n1 is the uncut run; a closed run followed by
    a frozen one is one run whose adaptation ends early.  A CLOSED first part cannot be continued: the iterate is gone."""
    spec, n, dim, n1, n2, L = energy_spec(kind, 5), 9, 5, 4, 7, 3
    eps = 2.0 * step_size(kind, dim)
    x0 = torch.randn(n, dim, generator=_gen(5))
    s = ta.GeneralizedHMC(model_of(spec), step_size=eps, n_leapfrog_steps=L, friction=GAMMA, temperature=TEMP)
    mu = math.log(10.0 * eps)
    args = (eps, GAMMA, TEMP, L, 0.8, mu, (1e-6, 1e3))
    whole = adapt.eager_adapt(s, x0, None, n1 + n2, n1 + n2, *args, adapt.da_table(n1 + n2), _gen(12))
    g = _gen(12)
    x, v, da, a1 = adapt.eager_adapt(s, x0, None, n1, n1, *args, adapt.da_table(n1), g, close=False)
    x, v, da, a2 = adapt.eager_adapt(s, x, v, n2, n2, *args, adapt.da_table(n2, n1), g, da=da)
    for got, want in zip((x, v, da), whole):
        assert torch.equal(got, want)
    assert torch.allclose((n1 * a1 + n2 * a2) / (n1 + n2), whole[3], rtol=1e-6)
    # closed, then frozen
    whole = adapt.eager_adapt(s, x0, None, n1, n1 + n2, *args, adapt.da_table(n1), _gen(12))
    g = _gen(12)
    x, v, da, _ = adapt.eager_adapt(s, x0, None, n1, n1, *args, adapt.da_table(n1), g)
    x, v, da2, _ = adapt.eager_adapt(s, x, v, 0, n2, *args, adapt.da_table(0), g, da=da)
    assert torch.equal(da2, da) and torch.equal(x, whole[0]) and torch.equal(v, whole[1]) and torch.equal(da, whole[2])
    # and the restatement agrees with both
    xi0, z, u = _replay(12, n, dim, n1 + n2)
    ref = restate(oracle_of(spec), x0, None, z, u, eps, L, GAMMA, TEMP, xi0=xi0, n_adapt=n1)
    assert torch.equal(x, ref["x"]) and torch.equal(da, ref["da"])


def test_apply_sets_the_step_size():
    s = ta.GeneralizedHMC(ta.HarmonicModel(k=4.0), step_size=0.05, n_leapfrog_steps=4, friction=math.inf)
    g = _gen(0)
    r = s.adapt_step_size(x=0.5 * torch.randn(512, 4, generator=g), n_steps=60, generator=g)
    assert isinstance(r, ta.samplers.StepSizeAdaptation) and r.step_sizes.shape == r.acceptance.shape == (512,)
    assert s.get_scheduled_value("step_size") == float(r.step_size) and s.schedulers["step_size"].is_constant()
    assert 4.0 * 0.05 < float(r.step_size) < 1.0  # it grew from a start that accepted everything
    assert 0.6 < r.acceptance.mean().item() < 0.95
    # a production run at the adapted step accepts (no equality with the target: the averaged iterate is not the last one)
    _, diag = s.sample(x=r.x, n_steps=20, return_diagnostics=True, generator=g)
    assert 0.6 < diag["acceptance_rate"].mean().item() <= 1.0
    # a scheduler is replaced by the constant
    sched = ta.HamiltonianMonteCarlo(ta.HarmonicModel(k=4.0), step_size=ta.core.schedules.LinearScheduler(0.3, 0.1, 10), n_leapfrog_steps=2)
    r = sched.adapt_step_size(dim=3, n_samples=64, n_steps=20, generator=_gen(1))
    assert sched.schedulers["step_size"].is_constant() and sched.get_scheduled_value("step_size") == float(r.step_size)


def test_validation_and_routing():
    m = ta.DoubleWellModel()
    s = ta.GeneralizedHMC(m, step_size=0.05)
    x = torch.zeros(3, 2)
    for kw, match in ((dict(n_steps=0), "n_steps"), (dict(target_accept=0.0), "target_accept"), (dict(target_accept=1.0), "target_accept"),
                      (dict(init_step_size=0.0), "init_step_size"), (dict(init_step_size=math.inf), "init_step_size"),
                      (dict(gamma=0.0), "gamma"), (dict(kappa=-1.0), "kappa"), (dict(mu_factor=0.0), "mu_factor"),
                      (dict(bounds=(0.0, 1.0)), "bounds"), (dict(bounds=(2.0, 1.0)), "bounds"),
                      (dict(velocity=torch.zeros(3, 3)), "velocity must have the state's shape")):
        with pytest.raises(ValueError, match=match):
            s.adapt_step_size(x=x, **kw)
    with pytest.raises(ValueError, match="dim must be provided"):
        s.adapt_step_size()
    with pytest.raises(ValueError, match="mass tensor must have"):
        ta.GeneralizedHMC(m, step_size=0.05, mass=torch.ones(3)).adapt_step_size(x=x)
    assert s.get_scheduled_value("step_size") == 0.05
    assert adapt.adapt_route(s, x, 1.0) == ("eager", None)

    class AsCuda:  # what the routing reads of a state, with no GPU at hand
        def __init__(self, dim, dtype=torch.float32, ndim=2):
            self.is_cuda, self.dtype, self.ndim, self.shape, self.device = True, dtype, ndim, (8, dim), torch.device("cpu")

    hmc = ta.HamiltonianMonteCarlo(m, step_size=0.05, n_leapfrog_steps=2)
    for smp in (s, hmc):
        assert adapt.adapt_route(smp, AsCuda(256), 1.0)[0] == "fused" and adapt.adapt_route(smp, AsCuda(2), 1.0)[0] == "fused"
        assert adapt.adapt_route(smp, AsCuda(257), 1.0)[0] == "eager" and adapt.adapt_route(smp, AsCuda(8, torch.float64), 1.0)[0] == "eager"
    sched = ta.core.schedules.LinearScheduler(0.3, 0.1, 10)
    for smp in (ta.GeneralizedHMC(m, step_size=0.05, mass=2.0), ta.HamiltonianMonteCarlo(m, step_size=0.05, mass=2.0),
                ta.GeneralizedHMC(m, step_size=sched), ta.HamiltonianMonteCarlo(m, step_size=sched),
                ta.GeneralizedHMC(ta.MLPEnergy(8, 64), step_size=0.01), ta.HamiltonianMonteCarlo(ta.MLPEnergy(8, 64), step_size=0.01)):
        assert adapt.adapt_route(smp, AsCuda(8), 1.0)[0] == "eager"
    # the eager route runs a mass, a scheduler, an nn.Module energy, and never reaches the entry
    before = hip_calls(ENTRY)

    class Quartic(ta.BaseModel):
        def forward(self, x):
            return (x**4).sum(dim=-1)

    for smp in (ta.GeneralizedHMC(m, step_size=0.05, mass=2.0), ta.GeneralizedHMC(m, step_size=0.05, mass=torch.tensor([1.0, 2.0, 0.5])),
                ta.HamiltonianMonteCarlo(m, step_size=0.05, n_leapfrog_steps=2, mass=2.0), ta.GeneralizedHMC(m, step_size=sched),
                ta.GeneralizedHMC(Quartic(), step_size=0.05, n_leapfrog_steps=2)):
        r = smp.adapt_step_size(dim=3, n_samples=32, n_steps=12, generator=_gen(2))
        assert r.x.shape == r.velocity.shape == (32, 3) and torch.isfinite(r.step_sizes).all() and float(r.step_size) > 0
    assert hip_calls(ENTRY) == before


@pytest.mark.parametrize("which", ["ghmc", "hmc"])
def test_the_fused_route_is_one_recorded_launch(fused_cpu, monkeypatch, which):  # noqa: F811
    make, rec, _ = fused_cpu
    reserved = []
    monkeypatch.setattr(_rng, "reserve", lambda generator, device, n_steps: reserved.append(n_steps) or (7, 11))
    if which == "ghmc":
        s, gamma, temp = make(ta.GeneralizedHMC, step_size=0.05, n_leapfrog_steps=3, friction=1.5, temperature=0.8), 1.5, 0.8
    else:
        s, gamma, temp = make(ta.HamiltonianMonteCarlo, step_size=0.05, n_leapfrog_steps=3), math.inf, 1.0
    x0 = torch.randn(16, 4, generator=_gen(1))
    keep = x0.clone()
    r = s.adapt_step_size(x=x0, n_steps=5, target_accept=0.7, bounds=(1e-4, 10.0), apply=False)
    assert reserved == [2 * 5 + 1]
    assert [name for name, _ in rec.calls] == [ENTRY]
    a = rec.calls[0][1]
    assert len(a) == len(_lib._PROTOTYPES[ENTRY][1]) == 29
    assert a[1] == r.x.data_ptr() != x0.data_ptr() and a[2] == r.velocity.data_ptr() and torch.equal(x0, keep)
    assert tuple(a[3:14]) == (16, 4, 5, 3, 0.05, 0.7, math.log(10.0 * 0.05), 1e-4, 10.0, 5, _lib.DA_INIT)
    assert a[14] == r.da.data_ptr() and a[15] is not None and a[16] is None and a[17] == r.acceptance.data_ptr()
    assert tuple(a[18:]) == (gamma, temp, 1, 1, None, None, None, None, 7, 11, None)
    assert r.step_sizes.data_ptr() == r.da.data_ptr() and r.da.shape == (3, 16)
    # a passed velocity is copied and read (draw_v0 = 0); init_step_size takes the place of the sampler's
    rec.calls.clear()
    v0 = torch.ones(16, 4)
    r = s.adapt_step_size(x=x0, n_steps=5, velocity=v0, init_step_size=0.2, apply=False)
    a = rec.calls[0][1]
    assert a[2] == r.velocity.data_ptr() != v0.data_ptr() and torch.equal(v0, torch.ones(16, 4))
    assert a[7] == 0.2 and a[9] == math.log(2.0) and a[20] == 0 and len(rec.named(ENTRY)) == 1


# ---------------------------------------------------------------------------------
# the entry
# ---------------------------------------------------------------------------------
def _abi_call(desc, *, x=16, v=16, n=4, dim=8, n_mh=3, L=2, eps0=0.1, delta=0.8, mu=0.0, eps_min=1e-6, eps_max=1e3, n_adapt=3,
              init_da=1, da=16, table=16, trace=None, alpha=None, gamma=1.0, temp=1.0, thin=1, traj=None, mask=None):
    _lib.call(ENTRY, desc, x, v, n, dim, n_mh, L, eps0, delta, mu, eps_min, eps_max, n_adapt, init_da, da, table, trace, alpha, gamma, temp,
              0, thin, traj, mask, None, None, 0, 0, None)


REFUSALS = [
    (dict(dim=257), RuntimeError, r"code -3.*dim 257"),  # ebm_ghmc_chain_f32's, in its order
    (dict(dim=0), RuntimeError, r"code -3.*dim 0"),
    (dict(n_mh=0, n_adapt=0), ValueError, "n_mh=0"),
    (dict(L=0), ValueError, "n_leapfrog=0"),
    (dict(thin=0), ValueError, "thin=0"),
    (dict(x=None), ValueError, "state pointer is NULL"),
    (dict(v=None), ValueError, "velocity pointer is NULL"),
    (dict(eps0=0.0), ValueError, "eps=0 "),
    (dict(eps0=float("nan")), ValueError, "eps=nan"),
    (dict(gamma=0.0), ValueError, "gamma=0 "),
    (dict(temp=float("nan")), ValueError, "temperature=nan"),
    (dict(da=None), ValueError, "da pointer is NULL"),  # the adaptation's own
    (dict(table=None), ValueError, "da_table pointer is NULL"),
    (dict(n_adapt=-1), ValueError, "n_adapt=-1"),
    (dict(n_adapt=4), ValueError, "n_adapt=4"),
    (dict(init_da=4), ValueError, "init_da=4"),
    (dict(delta=0.0), ValueError, "target_accept=0 "),
    (dict(delta=1.0), ValueError, "target_accept=1 "),
    (dict(delta=float("nan")), ValueError, "target_accept=nan"),
    (dict(eps_min=0.0), ValueError, "eps_min=0 "),
    (dict(eps_max=math.inf), ValueError, "eps_max=inf"),
    (dict(eps_min=2.0, eps_max=1.0), ValueError, "eps_min=2 eps_max=1 "),
    (dict(mu=math.inf), ValueError, "mu=inf"),
    (dict(mu=float("nan")), ValueError, "mu=nan"),
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
    _abi_call(desc, n=0, gamma=math.inf, n_adapt=0, table=None, init_da=2)  # ... and these are no refusals
    with pytest.raises(ValueError, match="da pointer is NULL"):
        _abi_call(desc, n=0, da=None)  # ... but the refusals come first


def test_the_entry_is_exported_and_declared():
    """Fails without the feature."""
    with open(os.path.join(INCLUDE, "ebm_hip.h")) as fh:
        header = fh.read()
    with open(os.path.join(INCLUDE, "ebm_hip_adapt.h")) as fh:
        companion = fh.read()
    assert '#include "ebm_hip.h"' in companion
    assert re.findall(r"EBM_API\s+int\s+(ebm_\w+)\s*\(", companion) == list(_lib.EXPORTS_ADAPT) == [ENTRY]

    def params(text, name):
        m = re.search(r"EBM_API\s+int\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        return re.sub(r"\s+", " ", m.group(1)).strip()

    eleven = ("double eps0, double target_accept, double mu, double eps_min, double eps_max, int32_t n_adapt, int32_t init_da, "
              "float* da, const float* da_table, float* eps_trace, float* alpha_mean, ")
    assert params(companion, ENTRY) == params(header, "ebm_ghmc_chain_f32").replace("double eps, ", eleven)
    proto, unit = _lib._PROTOTYPES[ENTRY][1], _lib._PROTOTYPES["ebm_ghmc_chain_f32"][1]
    assert proto == unit[:7] + [_lib._d] * 5 + [_lib._i32] * 2 + [_lib._p] * 4 + unit[8:]
    assert hasattr(_lib.lib(), ENTRY) and ENTRY not in _lib.EXPORTS and ENTRY not in _lib.EXPORTS_MASS_MLP
    assert _lib.ABI_VERSION == 9 and _lib.lib().ebm_version() == 9 and len(_lib.EXPORTS) == 58
    assert (_lib.DA_INIT, _lib.DA_OPEN) == tuple(int(v) for v in re.findall(r"#define EBM_DA_(?:INIT|OPEN) (\d)", companion))
    for text in ("m = m0 + t + 1", "w = 1 / (m + t0)", "s = sqrt(m) / gamma_da", "k = m^(-kappa)"):  # the header states the table
        assert text in companion
