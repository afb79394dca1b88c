"""ebm_kinetic_moments_mlp_f32 and the route of sample_moments to it, on the CPU: the export, its declaration and prototype, the
refusals in front of any device access, the second opt-in ``fused_mlp_moments`` (off by default, nothing on the CPU), the fused call
against the recorder, and the cases of test_kinetic_moments_mlp_gpu.py themselves (margins, seeds, decisions, the fp32
restatement's own error)."""

import math
import os
import re

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import fused_cpu  # noqa: F401
from kinetic_moments_mlp_cases import (BAOAB_CASES, GHMC_CASES, MARGIN_BAR, MAX_SEEDS, MIN_DECISIONS, baoab_case, ghmc_case,
                                       restatement_errors)

ENTRY = "ebm_kinetic_moments_mlp_f32"
ANALYTIC = "ebm_kinetic_moments_f32"
PLAIN = ("ebm_kinetic_mlp_chain_f32", "ebm_ghmc_mlp_chain_f32")
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
    assert ENTRY in _lib.EXPORTS and ENTRY in _lib._PROTOTYPES
    assert _lib._PROTOTYPES[ENTRY] == _lib._PROTOTYPES[ANALYTIC] and len(_lib._PROTOTYPES[ENTRY][1]) == 27
    with open(HEADER) as fh:
        header = fh.read()
    assert _parameter_list(header, ENTRY) == _parameter_list(header, ANALYTIC)
    assert _lib.ABI_VERSION == 9
    assert hasattr(_lib.lib(), ENTRY)


# ---------------------------------------------------------------------------------
# the entry's refusals, in front of any device access
# ---------------------------------------------------------------------------------
def _mlp_desc(hidden):
    desc = _lib.EnergyDesc()
    desc.kind, desc.n_comp, desc.dev0 = _lib.ENERGY_MLP, hidden, 16
    return desc


def _abi_call(desc, *, entry=ENTRY, x=16, v=16, n=4, dim=8, sampler=0, k=8, burn_in=0, L=2, step=0.1, gamma=1.0, temp=1.0, recip=16,
              mom=16, v2_mom=None, v_traj=None):
    _lib.call(entry, desc, x, v, n, dim, sampler, k, burn_in, L, step, gamma, temp, 0, recip, mom, None, v2_mom, None, None, v_traj,
              None, None, None, None, 0, 0, None)


EINVAL = [
    (dict(x=None), "state pointer is NULL"),
    (dict(v=None), "velocity pointer is NULL"),
    (dict(mom=None), "recip / mom is NULL"),
    (dict(recip=None), "recip / mom is NULL"),
    (dict(sampler=2), "sampler=2"),
    (dict(sampler=-1), "sampler=-1"),
    (dict(k=7), "k_steps=7 burn_in=0"),
    (dict(k=2), "k_steps=2 burn_in=0"),
    (dict(k=8, burn_in=6), "k_steps=8 burn_in=6"),
    (dict(k=8, burn_in=-2), "burn_in=-2"),
    (dict(k=4, burn_in=8), "k_steps=4 burn_in=8"),
    (dict(step=0.0), "step=0 "),
    (dict(step=-0.1), "step=-0.1"),
    (dict(step=NAN), "step=nan"),
    (dict(step=INF), "step=inf"),
    (dict(sampler=1, step=INF), "step=inf"),
    (dict(gamma=0.0), "gamma=0 "),
    (dict(gamma=-1.0), "gamma=-1"),
    (dict(gamma=NAN), "gamma=nan"),
    (dict(gamma=INF), "gamma=inf"),  # BAOAB: finite
    (dict(sampler=1, gamma=NAN), "gamma=nan"),
    (dict(temp=0.0), "temperature=0 "),
    (dict(temp=NAN), "temperature=nan"),
    (dict(temp=INF), "temperature=inf"),
    (dict(sampler=1, temp=INF), "temperature=inf"),
    (dict(sampler=1, L=0), "n_leapfrog=0"),
    (dict(sampler=1, v2_mom=16), "v2_mom / v_traj"),
    (dict(sampler=1, v_traj=16), "v2_mom / v_traj"),
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
            for sampler in (0, 1):
                with pytest.raises(RuntimeError, match=r"code -2.*MLP energy only"):  # EBM_EKIND
                    _abi_call(other, n=n, sampler=sampler)
        for sampler in (0, 1):  # EBM_EDIM: the message names both numbers
            with pytest.raises(RuntimeError, match=r"code -3.*hidden width 64 or 128.*got 96, 8"):
                _abi_call(_mlp_desc(96), n=n, sampler=sampler)
            with pytest.raises(RuntimeError, match=r"code -3.*hidden width 64 or 128.*got 256, 8"):
                _abi_call(_mlp_desc(256), n=n, sampler=sampler)
            with pytest.raises(RuntimeError, match=r"code -3.*1 <= dim <= 128.*got 64, 129"):
                _abi_call(desc, n=n, dim=129, sampler=sampler)
            with pytest.raises(RuntimeError, match=r"code -3.*got 128, 0"):
                _abi_call(_mlp_desc(128), n=n, dim=0, sampler=sampler)
    with pytest.raises(ValueError, match="bad shape"):
        _abi_call(desc, n=-1)
    _abi_call(desc, n=0)  # an empty call returns in front of any launch
    _abi_call(desc, n=0, sampler=1, gamma=INF)  # ... and an infinite friction is no refusal for generalized HMC
    _abi_call(desc, n=0, L=0)  # ... nor is n_leapfrog for BAOAB, which ignores it
    _abi_call(desc, n=0, v2_mom=16, v_traj=16)  # ... nor BAOAB's own outputs
    _abi_call(_mlp_desc(128), n=0, dim=128, k=11, burn_in=3, sampler=1, L=5)
    # ebm_kinetic_moments_f32 is untouched: it still refuses the MLP
    for n in (4, 0):
        with pytest.raises(RuntimeError, match=r"code -2.*no running-moments kernel"):
            _abi_call(desc, entry=ANALYTIC, n=n)


# ---------------------------------------------------------------------------------
# the second opt-in
# ---------------------------------------------------------------------------------
def test_the_second_opt_in_is_off_by_default():
    assert ta.UnderdampedLangevin.fused_mlp_moments is False and ta.GeneralizedHMC.fused_mlp_moments is False
    assert ta.UnderdampedLangevin(ta.MLPEnergy(3, 64), step_size=0.1).fused_mlp_moments is False
    assert ta.GeneralizedHMC(ta.MLPEnergy(3, 64), step_size=0.1).fused_mlp_moments is False


@pytest.mark.parametrize("which", ["baoab", "ghmc"])
def test_on_the_cpu_both_opt_ins_change_nothing(which):
    torch.manual_seed(4)
    model = ta.MLPEnergy(4, 64)
    if which == "baoab":
        make = lambda: ta.UnderdampedLangevin(model, step_size=0.2, friction=1.5, temperature=0.8)  # noqa: E731
    else:
        make = lambda: ta.GeneralizedHMC(model, step_size=0.4, n_leapfrog_steps=2, friction=1.5, temperature=0.8)  # noqa: E731
    plain, opted = make(), make()
    opted.fused_mlp = opted.fused_mlp_moments = True
    x0 = torch.randn(24, 4, generator=_gen(1))
    assert opted._route(x0)[0] == "eager"  # CPU states
    before = {name: _lib.call_counts[name] for name in (ENTRY, *PLAIN)}
    xa, a, va = plain.sample_moments(x=x0, n_steps=9, burn_in=1, energy=True, return_velocity=True, generator=_gen(9))
    xb, b, vb = opted.sample_moments(x=x0, n_steps=9, burn_in=1, energy=True, return_velocity=True, generator=_gen(9))
    assert {name: _lib.call_counts[name] for name in (ENTRY, *PLAIN)} == before
    assert torch.equal(xa, xb) and torch.equal(va, vb)
    assert torch.equal(a.chain_mean, b.chain_mean) and torch.equal(a.chain_m2, b.chain_m2)
    assert torch.equal(a.energy_mean, b.energy_mean) and torch.equal(a.energy_m2, b.energy_m2)
    if which == "baoab":
        assert torch.equal(a.velocity_sq_mean, b.velocity_sq_mean)
    else:
        assert torch.equal(a.acceptance_rate, b.acceptance_rate)


# ---------------------------------------------------------------------------------
# routing: the fused call against the recorder
# ---------------------------------------------------------------------------------
def _mlp_sampler(make, monkeypatch, which, moments=True, **kw):
    """A sampler on an MLPEnergy(5, 64) whose ``_route`` says "fused_mlp" on CPU tensors, as it would for CUDA ones."""
    torch.manual_seed(8)
    model = ta.MLPEnergy(5, 64)
    if which == "baoab":
        s = make(ta.UnderdampedLangevin, model=ta.DoubleWellModel(), **kw)
    else:
        s = make(ta.GeneralizedHMC, model=ta.DoubleWellModel(), n_leapfrog_steps=3, **kw)
    s.model, s.fused_mlp = model, True
    if moments:
        s.fused_mlp_moments = True
    spec = ta.core.energies.FusedSpec(_lib.ENERGY_MLP, n_comp=64, dev0=model._packed_parameters(), langevin_only=True, dim=5, hmc=True)
    monkeypatch.setattr(s, "_route", lambda x, model_kwargs=None: ("fused_mlp", spec))
    return s


@pytest.mark.parametrize("which", ["baoab", "ghmc"])
def test_the_route_is_one_call_of_the_entry(fused_cpu, monkeypatch, which):  # noqa: F811
    """Fails without the feature: sample_moments of such a sampler loops over sample(n_steps=1)."""
    make, rec, _ = fused_cpu
    s = _mlp_sampler(make, monkeypatch, which, step_size=0.2, friction=1.5, temperature=0.8)
    x0, v0 = torch.randn(6, 5, generator=_gen(0)), torch.randn(6, 5, generator=_gen(1))
    keep_x, keep_v = x0.clone(), v0.clone()
    x, mom, v = s.sample_moments(x=x0, n_steps=11, burn_in=2, energy=True, velocity=v0, return_velocity=True)
    assert [name for name, _ in rec.calls] == [ENTRY] and dict(_lib.call_counts) == {ENTRY: 1}
    a = rec.calls[0][1]
    assert len(a) == len(_lib._PROTOTYPES[ENTRY][1]) == 27
    assert a[0].kind == _lib.ENERGY_MLP and a[0].n_comp == 64
    assert a[1] == x.data_ptr() and a[2] == v.data_ptr() and a[3:6] == (6, 5, 0 if which == "baoab" else 1)
    assert a[6:9] == (11, 3, 0 if which == "baoab" else 3)  # the odd count burnt one more step
    assert a[9:12] == (0.2, 1.5, 0.8) and a[12] == 0  # velocities were passed: none is drawn
    assert a[13] is not None and a[14] is not None and a[15] is not None
    assert (a[16] is not None) == (which == "baoab")  # v2_mom
    # no trajectory pointer; generalized HMC's acceptance comes from the accept mask, not from the shared counters
    assert a[17:20] == (None, None, None) and (a[20] is not None) == (which == "ghmc") and a[21:24] == (None, None, None)
    assert a[24:26] == (7, 11)
    assert torch.equal(x0, keep_x) and torch.equal(v0, keep_v)
    assert x.data_ptr() != x0.data_ptr() and v.data_ptr() != v0.data_ptr()
    assert mom.half_len == 4 and mom.chain_mean.shape == (2, 6, 5) and mom.energy_mean.shape == (2, 6)
    assert (mom.velocity_sq_mean is not None) == (which == "baoab") and (mom.acceptance_rate is not None) == (which == "ghmc")
    # no velocity: the entry draws it; no energy: no e_mom
    rec.calls.clear()
    s.sample_moments(x=x0, n_steps=8)
    a = rec.calls[0][1]
    assert [name for name, _ in rec.calls] == [ENTRY] and a[12] == 1 and a[15] is None and a[6:8] == (8, 0)


def test_generalized_hmc_passes_an_infinite_friction(fused_cpu, monkeypatch):  # noqa: F811
    make, rec, _ = fused_cpu
    s = _mlp_sampler(make, monkeypatch, "ghmc", step_size=0.2, friction=INF)
    s.sample_moments(x=torch.zeros(6, 5), n_steps=8)
    assert [name for name, _ in rec.calls] == [ENTRY] and rec.calls[0][1][10] == INF


@pytest.mark.parametrize("which", ["baoab", "ghmc"])
def test_with_fused_mlp_alone_the_entry_is_not_called(fused_cpu, monkeypatch, which):  # noqa: F811
    """The step-by-step recurrence stays: one call of the sampler's plain MLP entry per transition, none of the new one."""
    make, rec, _ = fused_cpu
    s = _mlp_sampler(make, monkeypatch, which, moments=False, step_size=0.2)
    assert s.fused_mlp is True and s.fused_mlp_moments is False
    s.sample_moments(x=torch.randn(6, 5, generator=_gen(0)), n_steps=8)
    names = [name for name, _ in rec.calls]
    assert ENTRY not in names and ANALYTIC not in names
    assert names.count(PLAIN[0 if which == "baoab" else 1]) == 8


def test_the_reserved_philox_steps_are_samples(fused_cpu, monkeypatch):  # noqa: F811
    make, rec, _ = fused_cpu
    asked = []
    monkeypatch.setattr(_rng, "reserve", lambda generator, device, n_steps: asked.append(n_steps) or (7, 11))
    x0 = torch.randn(6, 5, generator=_gen(0))
    _mlp_sampler(make, monkeypatch, "baoab", step_size=0.2).sample_moments(x=x0, n_steps=10)
    _mlp_sampler(make, monkeypatch, "ghmc", step_size=0.2).sample_moments(x=x0, n_steps=10)
    assert asked == [11, 21] and [name for name, _ in rec.calls] == [ENTRY, ENTRY]


@pytest.mark.parametrize("which", ["baoab", "ghmc"])
def test_a_failing_launch_raises_and_nothing_falls_back(fused_cpu, monkeypatch, which):  # noqa: F811
    make, rec, _ = fused_cpu
    rec.fail_on = ENTRY
    s = _mlp_sampler(make, monkeypatch, which, step_size=0.2)
    with pytest.raises(RuntimeError, match="failed"):
        s.sample_moments(x=torch.zeros(4, 5), n_steps=8)
    assert [name for name, _ in rec.calls] == [ENTRY]


def test_a_mask_too_large_falls_to_the_entrys_counters(fused_cpu, monkeypatch):  # noqa: F811
    from torchebm_amd.samplers import kinetic_moments

    make, rec, _ = fused_cpu
    monkeypatch.setattr(kinetic_moments, "MASK_MAX_BYTES", 8 * 6 - 1)
    s = _mlp_sampler(make, monkeypatch, "ghmc", step_size=0.2)
    _, mom = s.sample_moments(x=torch.zeros(6, 5), n_steps=8)
    a = rec.calls[0][1]
    assert [name for name, _ in rec.calls] == [ENTRY]
    assert a[20] is None and a[21] is not None and mom.acceptance_rate.shape == (8,)
    assert bool((mom.acceptance_rate == 0).all())  # the recorder launches nothing: the counters keep their zeros


# ---------------------------------------------------------------------------------
# the cases the GPU tests run
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,hidden,n,k,burn_in,L", GHMC_CASES)
def test_ghmc_cases_meet_their_conditions(in_dim, hidden, n, k, burn_in, L):
    """A seed among the first MAX_SEEDS, no fp64 decision closer than MARGIN_BAR to its threshold, the fp32 restatement decides
    alike, at least MIN_DECISIONS accepted and rejected decisions, and the fp32 restatement within 1e-4 x max |ref| of fp64."""
    c = ghmc_case(in_dim, hidden, n, k, burn_in, L)
    acc = c["ref64"]["accepted"]
    print(f"dim {in_dim} H {hidden} n {n} k {k} burn_in {burn_in} L {L}: seed {c['seed']}, margin {c['ref64']['margin']:.3e}, "
          f"rejected {int((~acc).sum())}, accepted {int(acc.sum())}")
    assert c["found"] and c["seed"] < MAX_SEEDS
    assert c["ref64"]["margin"] > MARGIN_BAR
    assert torch.equal(c["ref32"]["accepted"], acc) and acc.shape == (k, n)
    assert int(acc.sum()) >= MIN_DECISIONS and int((~acc).sum()) >= MIN_DECISIONS
    assert c["half"] == (k - burn_in) // 2 and c["ref64"]["traj"].shape == (n, 2 * c["half"], in_dim)
    for key, (err, scale) in restatement_errors(c, ("x", "v", "traj", "e_traj")).items():
        print(f"    {key}: fp32 restatement err {err:.3e}, max|ref| {scale:.3e}")
        assert err <= 1e-4 * scale, (key, err, scale)


@pytest.mark.parametrize("in_dim,hidden,n,k,burn_in", BAOAB_CASES)
def test_baoab_cases_meet_their_conditions(in_dim, hidden, n, k, burn_in):
    c = baoab_case(in_dim, hidden, n, k, burn_in)
    h = c["half"]
    assert (k, burn_in) in ((4, 0), (7, 3), (11, 3)) and h == (k - burn_in) // 2
    assert c["ref64"]["traj"].shape == c["ref64"]["v_traj"].shape == (n, 2 * h, in_dim) and c["ref64"]["e_traj"].shape == (n, 2 * h)
    for key, (err, scale) in restatement_errors(c, ("x", "v", "traj", "v_traj", "e_traj")).items():
        print(f"dim {in_dim} H {hidden} n {n} k {k} burn_in {burn_in}: {key} fp32 restatement err {err:.3e}, max|ref| {scale:.3e}")
        assert math.isfinite(err) and err <= 1e-4 * scale, (key, err, scale)
