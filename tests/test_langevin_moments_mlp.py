"""ebm_chain_moments_mlp_f32 and the route of LangevinDynamics.sample_moments to it, on the CPU: the export, its declaration and
prototype, the refusals in front of any device access, the opt-in ``fused_mlp_moments`` (off by default, nothing on the CPU), the
fused call against the recorder, the routing predicate, and the cases of test_langevin_moments_mlp_gpu.py themselves (the fp32
restatement's own error)."""

import math
import os
import re

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from torchebm_amd.samplers import moments
from helpers import fused_cpu  # noqa: F401
from langevin_moments_mlp_cases import CASES, case, restatement_errors

ENTRY = "ebm_chain_moments_mlp_f32"
ANALYTIC = "ebm_chain_moments_f32"
PLAIN = "ebm_langevin_chain_f32"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ebm_hip.h")
INF, NAN = float("inf"), float("nan")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _parameter_list(text, name):
    m = re.search(r"EBM_API\s+int\s+" + name + r"\s*\(([^)]*)\)", text)
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_the_entry_is_exported_and_declared():
    """Fails without the feature."""
    assert ENTRY in _lib.EXPORTS and ENTRY in _lib._PROTOTYPES
    assert _lib._PROTOTYPES[ENTRY] == _lib._PROTOTYPES[ANALYTIC] and len(_lib._PROTOTYPES[ENTRY][1]) == 24
    with open(HEADER) as fh:
        header = fh.read()
    assert _parameter_list(header, ENTRY) == _parameter_list(header, ANALYTIC)
    assert _lib.ABI_VERSION == 9 and _lib.lib().ebm_version() == 9
    assert hasattr(_lib.lib(), ENTRY)


# ---------------------------------------------------------------------------------
# the entry's refusals, in front of any device access
# ---------------------------------------------------------------------------------
def _mlp_desc(hidden):
    desc = _lib.EnergyDesc()
    desc.kind, desc.n_comp, desc.dev0 = _lib.ENERGY_MLP, hidden, 16
    return desc


def _abi_call(desc, *, entry=ENTRY, x=16, n=4, dim=8, sampler=0, k=8, burn_in=0, eta=0.05, sqrt_eta=0.2236, coef=1.4142, L=0, eps=0.0,
              recip=16, mom=16, e_mom=None, traj=None, e_traj=None, mask=None, counts=None, noise=None, u=None):
    _lib.call(entry, desc, x, n, dim, sampler, k, burn_in, eta, sqrt_eta, coef, L, eps, recip, mom, e_mom, traj, e_traj, mask, counts,
              noise, u, 0, 0, None)


EINVAL = [
    (dict(x=None), "state pointer is NULL"),
    (dict(mom=None), "recip / mom is NULL"),
    (dict(recip=None), "recip / mom is NULL"),
    (dict(sampler=1), "sampler=1.*ebm_kinetic_moments_mlp_f32"),
    (dict(sampler=2), "sampler=2"),
    (dict(sampler=-1), "sampler=-1"),
    (dict(k=7), "k_steps=7 burn_in=0"),
    (dict(k=2), "k_steps=2 burn_in=0"),
    (dict(k=8, burn_in=6), "k_steps=8 burn_in=6"),
    (dict(k=8, burn_in=-2), "burn_in=-2"),
    (dict(k=4, burn_in=8), "k_steps=4 burn_in=8"),
    (dict(eta=NAN), "eta=nan"),
    (dict(eta=INF), "eta=inf"),
    (dict(eta=-INF), "eta=-inf"),
    (dict(sqrt_eta=NAN), "sqrt_eta=nan"),
    (dict(sqrt_eta=INF), "sqrt_eta=inf"),
    (dict(coef=NAN), "noise_coef=nan"),
    (dict(coef=INF), "noise_coef=inf"),
]


def test_abi_refusals_need_no_gpu():
    """Every refusal comes in front of any device access (the pointers below are never dereferenced) and in front of the early
    return of an empty call."""
    desc = _mlp_desc(64)
    for n in (4, 0):
        with pytest.raises(ValueError, match="energy descriptor is NULL"):
            _abi_call(None, n=n)
        for kw, match in EINVAL:  # EBM_EINVAL
            with pytest.raises(ValueError, match=match):
                _abi_call(desc, n=n, **kw)
        for kind in (_lib.ENERGY_DOUBLE_WELL, _lib.ENERGY_HARMONIC, _lib.ENERGY_ROSENBROCK, _lib.ENERGY_ACKLEY, _lib.ENERGY_RASTRIGIN):
            other = _lib.EnergyDesc()
            other.kind = kind
            with pytest.raises(RuntimeError, match=r"code -2.*MLP energy only"):  # EBM_EKIND
                _abi_call(other, n=n)
        # EBM_EDIM: the message names both numbers
        with pytest.raises(RuntimeError, match=r"code -3.*hidden width 64 or 128.*got 96, 8"):
            _abi_call(_mlp_desc(96), n=n)
        with pytest.raises(RuntimeError, match=r"code -3.*hidden width 64 or 128.*got 256, 8"):
            _abi_call(_mlp_desc(256), n=n)
        with pytest.raises(RuntimeError, match=r"code -3.*1 <= dim <= 128.*got 64, 129"):
            _abi_call(desc, n=n, dim=129)
        with pytest.raises(RuntimeError, match=r"code -3.*got 128, 0"):
            _abi_call(_mlp_desc(128), n=n, dim=0)
    with pytest.raises(ValueError, match="bad shape"):
        _abi_call(desc, n=-1)
    _abi_call(desc, n=0)  # an empty call returns in front of any launch
    _abi_call(desc, n=0, L=-3, eps=NAN, mask=16, counts=16, u=16)  # ... and the HMC half of the parameter list is ignored
    _abi_call(desc, n=0, coef=0.0)  # ... and a noise-free walk is no refusal
    _abi_call(_mlp_desc(128), n=0, dim=128, k=11, burn_in=3)
    # ebm_chain_moments_f32 is untouched: it still refuses the MLP, under both samplers
    for n in (4, 0):
        for sampler in (0, 1):
            with pytest.raises(RuntimeError, match=r"code -2.*no running-moments kernel"):
                _abi_call(desc, entry=ANALYTIC, n=n, sampler=sampler, L=2, eps=0.1)


# ---------------------------------------------------------------------------------
# the opt-in
# ---------------------------------------------------------------------------------
def test_the_opt_in_is_off_by_default():
    assert ta.LangevinDynamics.fused_mlp_moments is False
    assert ta.LangevinDynamics(ta.MLPEnergy(3, 64), step_size=0.1).fused_mlp_moments is False


def test_on_the_cpu_the_opt_in_changes_nothing():
    torch.manual_seed(4)
    model = ta.MLPEnergy(4, 64)
    plain, opted = ta.LangevinDynamics(model, step_size=0.05), ta.LangevinDynamics(model, step_size=0.05)
    opted.fused_mlp_moments = True
    x0 = torch.randn(24, 4, generator=_gen(1))
    assert opted._route(x0, {})[0] == "eager"  # CPU states
    before = {name: _lib.call_counts[name] for name in (ENTRY, PLAIN, ANALYTIC)}
    xa, a = plain.sample_moments(x=x0, n_steps=9, burn_in=1, energy=True, generator=_gen(9))
    xb, b = opted.sample_moments(x=x0, n_steps=9, burn_in=1, energy=True, generator=_gen(9))
    assert {name: _lib.call_counts[name] for name in (ENTRY, PLAIN, ANALYTIC)} == before
    assert torch.equal(xa, xb)
    assert torch.equal(a.chain_mean, b.chain_mean) and torch.equal(a.chain_m2, b.chain_m2)
    assert torch.equal(a.energy_mean, b.energy_mean) and torch.equal(a.energy_m2, b.energy_m2)


def test_the_routing_predicate():
    ok = dict(opted_in=True, dtype=torch.float32, ndim=2, n=5, dim=6, route="fused", spec_kind=_lib.ENERGY_MLP, hidden=64, in_dim=6,
              constant=True, plain_integrator=True, autocast=False, has_clamp=False)
    assert moments.fused_mlp_moments_eligible(**ok)
    assert moments.fused_mlp_moments_eligible(**{**ok, "hidden": 128, "dim": 128, "in_dim": 128})
    for change in (dict(opted_in=False), dict(dtype=torch.float64), dict(ndim=3), dict(n=0), dict(route="step"), dict(route="eager"),
                   dict(spec_kind=_lib.ENERGY_GAUSSIAN), dict(spec_kind=None), dict(hidden=96), dict(hidden=256), dict(hidden=None),
                   dict(dim=129, in_dim=129), dict(dim=0, in_dim=0), dict(in_dim=7), dict(in_dim=None), dict(constant=False),
                   dict(plain_integrator=False), dict(autocast=True), dict(has_clamp=True)):
        assert not moments.fused_mlp_moments_eligible(**{**ok, **change}), change


# ---------------------------------------------------------------------------------
# routing: the fused call against the recorder
# ---------------------------------------------------------------------------------
def _mlp_sampler(make, monkeypatch, flag=True, hidden=64, in_dim=5, **kw):
    """A LangevinDynamics on an MLPEnergy(in_dim, hidden) whose ``_route`` says "fused" on CPU tensors, as it does for CUDA ones."""
    torch.manual_seed(8)
    model = ta.MLPEnergy(in_dim, hidden)
    s = make(ta.LangevinDynamics, model=ta.DoubleWellModel(), **kw)
    s.model = model
    if flag:
        s.fused_mlp_moments = True
    spec = ta.core.energies.FusedSpec(_lib.ENERGY_MLP, n_comp=hidden, dev0=model._packed_parameters(), langevin_only=True, dim=in_dim)
    monkeypatch.setattr(s, "_route", lambda x, model_kwargs=None: ("fused", spec))
    return s


def test_the_route_is_one_call_of_the_entry(fused_cpu, monkeypatch):  # noqa: F811
    """Fails without the feature: sample_moments of such a sampler loops over sample(n_steps=1)."""
    make, rec, _ = fused_cpu
    asked = []
    monkeypatch.setattr(_rng, "reserve", lambda generator, device, n_steps: asked.append(n_steps) or (7, 11))
    s = _mlp_sampler(make, monkeypatch, step_size=0.05, noise_scale=1.5)
    x0 = torch.randn(6, 5, generator=_gen(0))
    keep = x0.clone()
    x, mom = s.sample_moments(x=x0, n_steps=11, burn_in=2, energy=True)
    assert [name for name, _ in rec.calls] == [ENTRY] and dict(_lib.call_counts) == {ENTRY: 1}
    assert asked == [11]  # as sample(n_steps=11) reserves
    a = rec.calls[0][1]
    assert len(a) == len(_lib._PROTOTYPES[ENTRY][1]) == 24
    assert a[0].kind == _lib.ENERGY_MLP and a[0].n_comp == 64
    assert a[1] == x.data_ptr() and a[2:5] == (6, 5, 0)
    assert a[5:7] == (11, 3)  # the odd count burnt one more step
    assert a[7:10] == (0.05, 0.05**0.5, (2.0 * 1.5**2) ** 0.5)
    assert a[10:12] == (0, 0.0)
    assert a[12] is not None and a[13] is not None and a[14] is not None  # recip, mom, e_mom
    assert a[15:21] == (None,) * 6  # no trajectory, no mask, no counters, no injected draws
    assert a[21:23] == (7, 11)
    assert torch.equal(x0, keep) and x.data_ptr() != x0.data_ptr()  # the state was cloned: it aliased the caller's tensor
    assert mom.half_len == 4 and mom.chain_mean.shape == (2, 6, 5) and mom.energy_mean.shape == (2, 6)
    assert mom.acceptance_rate is None and mom.velocity_sq_mean is None
    assert s.schedulers["step_size"].step_count == 11 and s.schedulers["noise_scale"].step_count == 11  # advanced by k
    # no energy: no e_mom
    rec.calls.clear()
    s.sample_moments(x=x0, n_steps=8)
    a = rec.calls[0][1]
    assert [name for name, _ in rec.calls] == [ENTRY] and a[14] is None and a[5:7] == (8, 0)


def test_a_failing_launch_raises_and_nothing_falls_back(fused_cpu, monkeypatch):  # noqa: F811
    make, rec, _ = fused_cpu
    rec.fail_on = ENTRY
    s = _mlp_sampler(make, monkeypatch, step_size=0.05)
    with pytest.raises(RuntimeError, match="failed"):
        s.sample_moments(x=torch.zeros(4, 5), n_steps=8)
    assert [name for name, _ in rec.calls] == [ENTRY]


@pytest.mark.parametrize("why", ["no flag", "clamp", "scheduler", "heun", "hidden 96", "dim != in_dim", "float64", "empty"])
def test_off_the_eligible_calls_the_entry_is_not_called(fused_cpu, monkeypatch, why):  # noqa: F811
    """The step-by-step recurrence stays: one call of the sampler's plain entry per step, none of the new one."""
    make, rec, _ = fused_cpu
    kw, shape, n, dtype = dict(step_size=0.05), dict(), 6, torch.float32
    if why == "clamp":
        kw["clamp"] = (-3.0, 3.0)
    elif why == "scheduler":
        kw["step_size"] = ta.core.schedules.LinearScheduler(0.05, 0.01, 10)
    elif why == "heun":
        kw["integrator"] = "heun"
    elif why == "hidden 96":
        shape["hidden"] = 96
    elif why == "dim != in_dim":
        shape["in_dim"] = 7
    elif why == "float64":
        dtype = torch.float64
        kw["dtype"] = torch.float64
    elif why == "empty":
        n = 0
    s = _mlp_sampler(make, monkeypatch, flag=why != "no flag", **shape, **kw)
    assert s.fused_mlp_moments is (why != "no flag")
    s.sample_moments(x=torch.randn(n, 5, generator=_gen(0)).to(dtype), n_steps=8)
    names = [name for name, _ in rec.calls]
    assert ENTRY not in names and ANALYTIC not in names
    if why in ("no flag", "clamp", "scheduler", "hidden 96", "dim != in_dim"):  # the eager recurrence around sample(n_steps=1)
        assert len(rec.named("ebm_langevin_")) == 8


# ---------------------------------------------------------------------------------
# the cases the GPU tests run
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,hidden,n,k,burn_in", CASES)
def test_cases_meet_their_conditions(in_dim, hidden, n, k, burn_in):
    """The fp32 restatement within 1e-4 x max |ref| of fp64 (measured: within 6e-7 x on all 13 cases)."""
    c = case(in_dim, hidden, n, k, burn_in)
    h = c["half"]
    assert (k, burn_in) in ((4, 0), (7, 3), (11, 3)) and h == (k - burn_in) // 2
    assert c["ref64"]["x"].shape == (n, in_dim) and c["ref64"]["traj"].shape == (n, 2 * h, in_dim) and c["ref64"]["e_traj"].shape == (n, 2 * h)
    assert torch.equal(c["ref32"]["traj"][:, -1], c["ref32"]["x"])
    for key, (err, scale) in restatement_errors(c).items():
        print(f"dim {in_dim} H {hidden} n {n} k {k} burn_in {burn_in}: {key} fp32 restatement err {err:.3e}, max|ref| {scale:.3e}")
        assert math.isfinite(err) and err <= 1e-4 * scale, (key, err, scale)


def test_the_cases_cover_every_kernel():
    """Every (hidden, ceil(dim / 32)) instantiation, both Philox paths, a partial wave and several workgroups with a tail."""
    assert len(CASES) == 13
    assert {(c[1], (c[0] + 31) // 32) for c in CASES} == {(hid, dt) for hid in (64, 128) for dt in (1, 2, 3, 4)}
    assert any(c[0] % 4 for c in CASES) and any(c[0] % 4 == 0 for c in CASES)
    assert {c[2] for c in CASES} == {37, 129, 257} and {(c[3], c[4]) for c in CASES} == {(4, 0), (7, 3), (11, 3)}
