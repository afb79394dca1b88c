"""ebm_ghmc_mlp_chain_f32 and the ``fused_mlp`` opt-in of GeneralizedHMC without a GPU: the export and its declaration, the
refusals the entry makes in front of any device access, the shared request of the two GHMC entries, the opt-in's default and CPU
behaviour, ContrastiveDivergence with the opted-in sampler, the conditions every GPU case must meet, the fp32 restatement of every
case against fp64, and the one launch of the opted-in route against a recording stand-in of the library."""

import math
import os
import re

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from torchebm_amd.samplers.ghmc import ghmc_constants
from ghmc_mlp_cases import CASES, EPS, GAMMA, INF_CASE, MARGIN_BAR, MAX_SEEDS, MIN_DECISIONS, TEMP, case, constants, restatement_errors
from helpers import fused_cpu  # noqa: F401
from torchebm_amd.utils.synthetic import two_moons

ENTRY = "ebm_ghmc_mlp_chain_f32"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ebm_hip.h")
API = os.path.join(ROOT, "torchebm_amd", "csrc", "api.hip")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _parameter_list(text, name, prefix=r"EBM_API\s+int\s+"):
    """The parameter list of `name`'s declaration, white space collapsed."""
    m = re.search(prefix + name + r"\s*\(([^)]*)\)", text)
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_the_entry_is_exported_and_declared():
    assert ENTRY in _lib.EXPORTS and ENTRY in _lib._PROTOTYPES
    assert _lib._PROTOTYPES[ENTRY] == _lib._PROTOTYPES["ebm_ghmc_chain_f32"]  # the same parameter list
    with open(HEADER) as fh:
        header = fh.read()
    assert _parameter_list(header, ENTRY) == _parameter_list(header, "ebm_ghmc_chain_f32")
    assert _lib.ABI_VERSION == 9
    assert hasattr(_lib.lib(), ENTRY)


def _mlp_desc(hidden):
    desc = _lib.EnergyDesc()
    desc.kind, desc.n_comp, desc.dev0 = _lib.ENERGY_MLP, hidden, 16
    return desc


def _abi_call(desc, *, entry=ENTRY, x=16, v=16, n=4, dim=8, n_mh=3, L=2, eps=0.1, gamma=1.0, temp=1.0, thin=1):
    _lib.call(entry, desc, x, v, n, dim, n_mh, L, eps, gamma, temp, 0, thin, None, None, None, None, 0, 0, None)


INF, NAN = float("inf"), float("nan")
EINVAL = [
    (dict(x=None), "state pointer is NULL"),
    (dict(v=None), "velocity pointer is NULL"),
    (dict(n_mh=0), "n_mh=0"),
    (dict(L=0), "n_leapfrog=0"),
    (dict(thin=0), "thin=0"),
    (dict(eps=0.0), "eps=0 "),
    (dict(eps=-0.1), "eps=-0.1"),
    (dict(eps=INF), "eps=inf"),
    (dict(eps=NAN), "eps=nan"),
    (dict(gamma=0.0), "gamma=0 "),
    (dict(gamma=-1.0), "gamma=-1"),
    (dict(gamma=NAN), "gamma=nan"),
    (dict(temp=0.0), "temperature=0 "),
    (dict(temp=-2.0), "temperature=-2"),
    (dict(temp=INF), "temperature=inf"),
    (dict(temp=NAN), "temperature=nan"),
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
        with pytest.raises(RuntimeError, match=r"code -3.*hidden width 64 or 128.*got 96, 8"):  # EBM_EDIM
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
    _abi_call(desc, n=0, gamma=INF)  # ... and an infinite friction is no refusal
    _abi_call(_mlp_desc(128), n=0, dim=128, n_mh=7, thin=3, L=5)
    # ebm_ghmc_chain_f32 is untouched: it still refuses the MLP
    with pytest.raises(RuntimeError, match=r"code -2.*no generalized-HMC kernel"):
        _abi_call(desc, entry="ebm_ghmc_chain_f32")


def _c_double(expr, env):
    """A C expression of api.hip's ghmc_request in Python: double arithmetic, (float) rounds once."""
    expr = re.sub(r"std::isinf\(", "math.isinf(", expr)
    expr = re.sub(r"\(double\)", "", expr)
    expr = re.sub(r"(\d)f\b", r"\1", expr)
    m = re.match(r"(.*?)\?(.*?):(.*)$", expr)
    if m:
        return _c_double(m.group(2), env) if _c_double(m.group(1), env) else _c_double(m.group(3), env)
    m = re.match(r"\s*\(float\)(.*)$", expr)
    if m:
        return torch.tensor(_c_double(m.group(1), env), dtype=torch.float64).to(torch.float32).item()
    return eval(expr, {"math": math, "exp": math.exp, "sqrt": math.sqrt, "expm1": math.expm1, **env})  # noqa: S307


def test_both_ghmc_entries_form_their_constants_in_one_request():
    """ghmc_request is defined once, both entries call it and neither forms a constant itself; its expressions, read from the
    source and evaluated in double with (float) rounding once, are ghmc_constants' values -- also at gamma = inf."""
    with open(API) as fh:
        src = fh.read()
    assert len(re.findall(r"static\s+GhmcChainReq\s+ghmc_request\s*\(", src)) == 1
    body = re.search(r"static\s+GhmcChainReq\s+ghmc_request\s*\([^)]*\)\s*\{(.*?)\n\}", src, re.S).group(1)
    for entry, launch in (("ebm_ghmc_chain_f32", "ghmc_chain_launch"), ("ebm_ghmc_mlp_chain_f32", "ghmc_mlp_chain_launch")):
        text = re.search(r"\nint " + entry + r"\s*\([^)]*\)\s*\{(.*?)\n\}", src, re.S).group(1)
        assert re.search(launch + r"\(ghmc_request\(", text), entry
        assert "expm1" not in text and "sqrt(" not in text and "exp(" not in text, entry
    stmts = dict(re.findall(r"const (?:double|float) (\w+) = (.*?);", body))
    assert set(stmts) == {"span", "sqrt_temp", "c1", "c2", "beta"}
    assert re.search(r"n_leapfrog, \(float\)eps, c1, c2, sqrt_temp, beta,", body)
    for eps, L, gamma, temp in [(EPS, 3, GAMMA, TEMP), (0.05, 1, 1.0, 1.0), (0.3, 7, 0.25, 2.5), (1.0, 3, INF, TEMP), (1e-3, 1, 1e-4, 0.1)]:
        env = dict(eps=eps, n_leapfrog=L, gamma=gamma, temperature=temp)
        for name in ("span", "sqrt_temp", "c1", "c2", "beta"):  # (the order of the source)
            env[name] = _c_double(stmts[name], env)
        got = (env["c1"], env["c2"], env["sqrt_temp"], env["beta"])
        assert got == tuple(ghmc_constants(eps, L, gamma, temp)) == tuple(constants(eps, L, gamma, temp)), (eps, L, gamma, temp)


def test_the_opt_in_is_off_by_default_and_changes_nothing_on_the_cpu():
    assert ta.GeneralizedHMC.fused_mlp is False
    torch.manual_seed(4)
    model = ta.MLPEnergy(4, 64)
    kw = dict(step_size=0.4, n_leapfrog_steps=2, friction=1.5, temperature=0.8)
    plain, opted = ta.GeneralizedHMC(model, **kw), ta.GeneralizedHMC(model, **kw)
    assert plain.fused_mlp is False
    opted.fused_mlp = True
    x0 = torch.randn(48, 4, generator=_gen(1))
    assert plain._route(x0)[0] == "eager" and opted._route(x0)[0] == "eager" and opted._route(x0, {})[0] == "eager"  # CPU states
    a = plain.sample(x=x0, n_steps=7, thin=2, return_trajectory=True, return_diagnostics=True, return_velocity=True, generator=_gen(9))
    b = opted.sample(x=x0, n_steps=7, thin=2, return_trajectory=True, return_diagnostics=True, return_velocity=True, generator=_gen(9))
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and a[0].shape == (48, 3, 4)
    for key in ("mean", "var", "energy", "acceptance_rate", "kinetic_temperature"):
        assert torch.equal(a[1][key], b[1][key]), key
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[2]).all()


def test_sample_moments_of_an_opted_in_sampler_keeps_the_eager_recurrence():
    torch.manual_seed(5)
    model = ta.MLPEnergy(3, 64)
    kw = dict(step_size=0.3, n_leapfrog_steps=2, friction=1.0)
    plain, opted = ta.GeneralizedHMC(model, **kw), ta.GeneralizedHMC(model, **kw)
    opted.fused_mlp = True
    x0 = torch.randn(16, 3, generator=_gen(2))
    xa, ma = plain.sample_moments(x=x0, n_steps=12, burn_in=2, generator=_gen(3))
    xb, mb = opted.sample_moments(x=x0, n_steps=12, burn_in=2, generator=_gen(3))
    assert torch.equal(xa, xb) and torch.equal(ma.mean, mb.mean) and torch.equal(ma.acceptance_rate, mb.acceptance_rate)


@pytest.mark.parametrize("persistent", [False, True], ids=["cd_k", "persistent"])
def test_contrastive_divergence_takes_the_opted_in_sampler(persistent):
    torch.manual_seed(6)
    model = ta.MLPEnergy(2, 64)
    sampler = ta.GeneralizedHMC(model, step_size=0.1, n_leapfrog_steps=2, friction=1.0, temperature=1.0)
    sampler.fused_mlp = True  # eager on the CPU all the same
    cd = ta.losses.ContrastiveDivergence(model=model, sampler=sampler, k_steps=5, persistent=persistent, buffer_size=256, init_steps=0)
    data = two_moons(n_samples=64, noise=0.05, seed=0)
    for _ in range(2):  # (persistent: the second call starts from the buffer the first one wrote)
        model.zero_grad()
        loss, negatives = cd(data, generator=_gen(7))
        assert loss.ndim == 0 and torch.isfinite(loss)
        assert negatives.shape == data.shape and torch.isfinite(negatives).all() and not negatives.requires_grad
        loss.backward()
        grads = [p.grad for p in model.parameters()]
        assert all(g is not None and torch.isfinite(g).all() for g in grads) and any(g.abs().max() > 0 for g in grads)


ALL_CASES = [(*c, GAMMA) for c in CASES] + [(*INF_CASE, INF)]


@pytest.mark.parametrize("in_dim,hidden,n,n_mh,thin,L,gamma", ALL_CASES)
def test_every_case_decides_clearly_both_ways_and_its_fp32_restatement_tracks_fp64(in_dim, hidden, n, n_mh, thin, L, gamma):
    """The conditions of the GPU cases: a seed among the first MAX_SEEDS whose fp64 restatement has no decision within MARGIN_BAR
    of its threshold and whose fp32 restatement decides alike; at least MIN_DECISIONS accepted and as many rejected decisions (the
    flip runs); and chains that do not diverge -- the fp32 restatement's max error against fp64 is at most 1e-4 x max |ref| for x, v
    and the kept positions, so '4 x the fp32 restatement's own error' is a bar on round-off, not on chaos."""
    c = case(in_dim, hidden, n, n_mh, thin, L, gamma)
    acc = c["ref64"]["accepted"]
    n_acc, n_rej = int(acc.sum()), int((~acc).sum())
    print(f"dim {in_dim} H {hidden} n {n} n_mh {n_mh} L {L} gamma {gamma}: seed {c['seed']}, margin {c['ref64']['margin']:.2e}, "
          f"{n_acc} accepted, {n_rej} rejected ({n_rej / acc.numel():.1%})")
    assert c["found"] and c["seed"] < MAX_SEEDS
    assert c["ref64"]["margin"] > MARGIN_BAR and torch.equal(c["ref32"]["accepted"], acc)
    assert acc.shape == (n_mh, n) and n_acc >= MIN_DECISIONS and n_rej >= MIN_DECISIONS
    assert c["ref64"]["traj"].shape == (n, n_mh // thin, in_dim)
    for key, (err, scale) in restatement_errors(c).items():
        print(f"    {key} fp32 err {err:.3e} max|ref| {scale:.3e}")
        assert err <= 1e-4 * scale, (key, err, scale)


def _mlp_sampler(make, monkeypatch, **kw):
    model = ta.MLPEnergy(5, 64)
    s = make(ta.GeneralizedHMC, model=ta.DoubleWellModel(), **kw)
    s.model, s.fused_mlp = model, True
    spec = ta.core.energies.FusedSpec(_lib.ENERGY_MLP, n_comp=64, dev0=model._packed_parameters(), langevin_only=True, dim=5, hmc=True)
    monkeypatch.setattr(s, "_route", lambda x, model_kwargs: ("fused_mlp", spec))
    return s


def test_the_opted_in_route_is_one_launch_of_the_entry(fused_cpu, monkeypatch):  # noqa: F811
    make, rec, clones = fused_cpu
    torch.manual_seed(8)
    s = _mlp_sampler(make, monkeypatch, step_size=0.2, n_leapfrog_steps=3, friction=1.5, temperature=0.8)
    n, dim, k, thin = 37, 5, 11, 3
    x0, v0 = torch.randn(n, dim, generator=_gen(1)), torch.randn(n, dim, generator=_gen(2))
    x_before, v_before = x0.clone(), v0.clone()
    clones.clear()
    out = s.sample(x=x0, n_steps=k, thin=thin, generator=_gen(3))
    calls = rec.named("ebm_")
    assert [name for name, _ in calls] == [ENTRY]
    args = calls[0][1]
    assert out.data_ptr() == args[1] != x0.data_ptr() and x0.data_ptr() in clones
    # (energy, x, v, n, dim, n_mh, L, eps, gamma, T, draw_v0, thin, traj, mask, noise, u, seed, offset, stream)
    assert tuple(args[3:]) == (n, dim, k, 3, 0.2, 1.5, 0.8, 1, thin, None, None, None, None, 7, 11, None)
    assert torch.equal(x0, x_before)
    # velocities given: read, cloned, never the caller's; trajectory and diagnostics: the kept positions' buffer and the mask
    rec.calls.clear()
    traj, diag, v = s.sample(x=x0, n_steps=k, thin=thin, velocity=v0, return_trajectory=True, return_diagnostics=True,
                             return_velocity=True, generator=_gen(3))
    (name, args), = rec.named("ebm_")  # the statistics of the kept positions are torch ops: no further entry
    assert name == ENTRY and args[10] == 0 and args[2] == v.data_ptr() != v0.data_ptr()
    assert args[12] == traj.data_ptr() and traj.shape == (n, k // thin, dim) and args[13] is not None and args[14:16] == (None, None)
    assert diag["acceptance_rate"].shape == diag["energy"].shape == (k // thin,) and diag["mean"].shape == (k // thin, dim)
    assert torch.equal(v0, v_before) and torch.equal(x0, x_before)


def test_the_opted_in_route_reserves_two_steps_per_transition_and_one(fused_cpu, monkeypatch):  # noqa: F811
    make, rec, _ = fused_cpu
    s = _mlp_sampler(make, monkeypatch, step_size=0.2)
    reserved = []
    monkeypatch.setattr(_rng, "reserve", lambda generator, device, n_steps: reserved.append(n_steps) or (7, 11))
    s.sample(x=torch.zeros(8, 5), n_steps=9)
    assert reserved == [2 * 9 + 1] and [name for name, _ in rec.named("ebm_")] == [ENTRY]
    # no transition: no launch of the entry; the start velocities alone come from the noise field, as on the analytic fused route
    rec.calls.clear()
    x, v = s.sample(x=torch.ones(8, 5), n_steps=0, return_velocity=True)
    assert reserved == [19, 1]
    assert [name for name, _ in rec.named("ebm_")] == ["ebm_noise_fill_f32"] and torch.equal(x, torch.ones(8, 5)) and v.shape == (8, 5)
