"""ebm_kinetic_mlp_chain_f32, the ``fused_mlp`` opt-in of UnderdampedLangevin and ``model_kwargs`` on the two momentum samplers
without a GPU: the export and its declaration, the refusals the entry makes in front of any device access, the opt-in's default
and CPU behaviour, ContrastiveDivergence with both samplers, the fp32 restatement of every GPU case against fp64, and the one
launch of the opted-in route against a recording stand-in of the library."""

import os
import re

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib
from helpers import fused_cpu  # noqa: F401
from kinetic_mlp_cases import CASES, case, restatement_errors
from torchebm_amd.utils.synthetic import two_moons

ENTRY = "ebm_kinetic_mlp_chain_f32"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ebm_hip.h")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_the_entry_is_exported_and_declared():
    assert ENTRY in _lib.EXPORTS and ENTRY in _lib._PROTOTYPES
    assert _lib._PROTOTYPES[ENTRY] == _lib._PROTOTYPES["ebm_kinetic_chain_f32"]  # the same parameter list
    with open(HEADER) as fh:
        assert re.search(r"EBM_API\s+int\s+" + ENTRY + r"\s*\(", fh.read())
    assert _lib.ABI_VERSION == 9
    assert hasattr(_lib.lib(), ENTRY)


def _mlp_desc(hidden):
    desc = _lib.EnergyDesc()
    desc.kind, desc.n_comp, desc.dev0 = _lib.ENERGY_MLP, hidden, 16
    return desc


def _abi_call(desc, *, entry=ENTRY, x=16, v=16, n=4, dim=8, k=3, h=0.1, gamma=1.0, temp=1.0, thin=1):
    _lib.call(entry, desc, x, v, n, dim, k, h, gamma, temp, 0, thin, None, None, 0, 0, None)


INF, NAN = float("inf"), float("nan")
EINVAL = [
    (dict(x=None), "state pointer is NULL"),
    (dict(v=None), "velocity pointer is NULL"),
    (dict(k=0), "k_steps=0"),
    (dict(thin=0), "thin=0"),
    (dict(h=0.0), "h=0 "),
    (dict(h=-0.1), "h=-0.1"),
    (dict(h=INF), "h=inf"),
    (dict(h=NAN), "h=nan"),
    (dict(gamma=0.0), "gamma=0 "),
    (dict(gamma=-1.0), "gamma=-1"),
    (dict(gamma=INF), "gamma=inf"),
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
    _abi_call(desc, n=0)  # an empty call returns in front of any launch
    _abi_call(_mlp_desc(128), n=0, dim=128, k=7, thin=3)
    # ebm_kinetic_chain_f32 is untouched: it still refuses the MLP
    with pytest.raises(RuntimeError, match=r"code -2.*no underdamped-Langevin kernel"):
        _abi_call(desc, entry="ebm_kinetic_chain_f32")


def test_the_opt_in_is_off_by_default_and_changes_nothing_on_the_cpu():
    assert ta.UnderdampedLangevin.fused_mlp is False
    torch.manual_seed(4)
    model = ta.MLPEnergy(4, 64)
    kw = dict(step_size=0.2, friction=1.5, temperature=0.8)
    plain, opted = ta.UnderdampedLangevin(model, **kw), ta.UnderdampedLangevin(model, **kw)
    assert plain.fused_mlp is False
    opted.fused_mlp = True
    x0 = torch.randn(48, 4, generator=_gen(1))
    assert plain._route(x0)[0] == "eager" and opted._route(x0)[0] == "eager" and opted._route(x0, {})[0] == "eager"  # CPU states
    a = plain.sample(x=x0, n_steps=7, thin=2, return_trajectory=True, return_diagnostics=True, return_velocity=True, generator=_gen(9))
    b = opted.sample(x=x0, n_steps=7, thin=2, return_trajectory=True, return_diagnostics=True, return_velocity=True, generator=_gen(9))
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and a[0].shape == (48, 3, 4)
    for key in ("mean", "var", "energy", "kinetic_temperature"):
        assert torch.equal(a[1][key], b[1][key]), key
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[2]).all()


@pytest.mark.parametrize("cls,extra", [(ta.UnderdampedLangevin, {}), (ta.GeneralizedHMC, dict(n_leapfrog_steps=3))])
def test_empty_model_kwargs_change_nothing(cls, extra):
    torch.manual_seed(5)
    s = cls(ta.MLPEnergy(3, 64), step_size=0.2, friction=1.5, temperature=0.8, **extra)
    x0 = torch.randn(33, 3, generator=_gen(2))
    want = s.sample(x=x0, n_steps=6, thin=2, return_trajectory=True, return_velocity=True, generator=_gen(3))
    for kwargs in (None, {}):
        got = s.sample(x=x0, n_steps=6, thin=2, return_trajectory=True, return_velocity=True, model_kwargs=kwargs, generator=_gen(3))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(TypeError, match="model_kwargs must be a dict"):
        s.sample(x=x0, n_steps=1, model_kwargs=[1])


class _Tilted(ta.BaseModel):
    """E(x; shift) = 0.5 |x - shift|^2: conditioning that moves the well."""

    def forward(self, x, shift=None):
        return 0.5 * ((x - (0.0 if shift is None else shift)) ** 2).sum(dim=-1)


@pytest.mark.parametrize("cls,extra", [(ta.UnderdampedLangevin, {}), (ta.GeneralizedHMC, dict(n_leapfrog_steps=2))])
def test_model_kwargs_reach_the_model_on_the_eager_route(cls, extra):
    s = cls(_Tilted(), step_size=0.3, friction=2.0, temperature=0.05, **extra)
    x0 = torch.zeros(512, 2)
    shift = torch.tensor([3.0, -2.0])
    assert s._route(x0, {"shift": shift})[0] == "eager"
    out = s.sample(x=x0, n_steps=120, model_kwargs={"shift": shift}, generator=_gen(4))
    assert torch.allclose(out.mean(dim=0), shift, atol=0.1), out.mean(dim=0)
    plain = s.sample(x=x0, n_steps=120, generator=_gen(4))
    assert torch.allclose(plain.mean(dim=0), torch.zeros(2), atol=0.1)


@pytest.mark.parametrize("persistent", [False, True], ids=["cd_k", "persistent"])
@pytest.mark.parametrize("cls,extra", [(ta.UnderdampedLangevin, {}), (ta.GeneralizedHMC, dict(n_leapfrog_steps=2))],
                         ids=["kinetic", "ghmc"])
def test_contrastive_divergence_takes_the_momentum_samplers(cls, extra, persistent):
    torch.manual_seed(6)
    model = ta.MLPEnergy(2, 64)
    sampler = cls(model, step_size=0.1, friction=1.0, temperature=1.0, **extra)
    if cls is ta.UnderdampedLangevin:
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


@pytest.mark.parametrize("in_dim,hidden,n,k,thin", CASES)
def test_the_fp32_restatement_of_every_case_tracks_fp64(in_dim, hidden, n, k, thin):
    """The chains of the GPU cases do not diverge: the fp32 restatement's max error against fp64 is at most 1e-4 x max |ref| for
    x, v and the kept positions, so '4 x the fp32 restatement's own error' is a bar on round-off, not on chaos."""
    c = case(in_dim, hidden, n, k, thin)
    assert c["ref64"]["traj"].shape == (n, k // thin, in_dim)
    for key, (err, scale) in restatement_errors(c).items():
        print(f"dim {in_dim} H {hidden} n {n} k {k}: {key} fp32 err {err:.3e} max|ref| {scale:.3e}")
        assert err <= 1e-4 * scale, (key, err, scale)


def test_the_opted_in_route_is_one_launch_of_the_entry(fused_cpu, monkeypatch):  # noqa: F811
    make, rec, clones = fused_cpu
    torch.manual_seed(8)
    model = ta.MLPEnergy(5, 64)
    s = make(ta.UnderdampedLangevin, model=ta.DoubleWellModel(), step_size=0.2, friction=1.5, temperature=0.8)
    s.model = model
    s.fused_mlp = True
    spec = ta.core.energies.FusedSpec(_lib.ENERGY_MLP, n_comp=64, dev0=model._packed_parameters(), langevin_only=True, dim=5, hmc=True)
    monkeypatch.setattr(s, "_route", lambda x, model_kwargs: ("fused_mlp", spec))
    n, dim, k, thin = 37, 5, 11, 3
    x0, v0 = torch.randn(n, dim, generator=_gen(1)), torch.randn(n, dim, generator=_gen(2))
    x_before, v_before = x0.clone(), v0.clone()
    clones.clear()
    out = s.sample(x=x0, n_steps=k, thin=thin, generator=_gen(3))
    calls = rec.named("ebm_")
    assert [name for name, _ in calls] == [ENTRY]
    args = calls[0][1]
    state_ptr, vel_ptr = args[1], args[2]
    assert out.data_ptr() == state_ptr and state_ptr != x0.data_ptr() and x0.data_ptr() in clones
    # (energy, x, v, n, dim, k, h, gamma, T, draw_v0, thin, traj, noise, seed, offset, stream)
    assert list(args[3:6]) == [n, dim, k]
    assert list(args[6:9]) == [0.2, 1.5, 0.8]
    assert args[9] == 1 and args[10] == thin and args[11] is None and args[12] is None
    assert (args[13], args[14]) == (7, 11)  # the reserved Philox coordinates
    assert torch.equal(x0, x_before)
    # velocities given: read, cloned, never the caller's; a trajectory is asked for: the kept positions' buffer is passed
    rec.calls.clear()
    traj, v = s.sample(x=x0, n_steps=k, thin=thin, velocity=v0, return_trajectory=True, return_velocity=True, generator=_gen(3))
    (name, args), = rec.named("ebm_")
    assert name == ENTRY and args[9] == 0 and args[2] == v.data_ptr() != v0.data_ptr()
    assert args[11] == traj.data_ptr() and traj.shape == (n, k // thin, dim)
    assert torch.equal(v0, v_before) and torch.equal(x0, x_before)


def test_the_opted_in_route_reserves_one_step_more_than_it_takes(fused_cpu, monkeypatch):  # noqa: F811
    from torchebm_amd import _rng

    make, rec, _ = fused_cpu
    model = ta.MLPEnergy(5, 64)
    s = make(ta.UnderdampedLangevin, model=ta.DoubleWellModel(), step_size=0.2)
    s.model, s.fused_mlp = model, True
    spec = ta.core.energies.FusedSpec(_lib.ENERGY_MLP, n_comp=64, dev0=model._packed_parameters(), langevin_only=True, dim=5, hmc=True)
    monkeypatch.setattr(s, "_route", lambda x, model_kwargs: ("fused_mlp", spec))
    reserved = []
    monkeypatch.setattr(_rng, "reserve", lambda generator, device, n_steps: reserved.append(n_steps) or (7, 11))
    s.sample(x=torch.zeros(8, 5), n_steps=9)
    assert reserved == [10] and [name for name, _ in rec.named("ebm_")] == [ENTRY]
    # no step: no launch of the entry; the start velocities alone come from the noise field, as on the analytic fused route
    rec.calls.clear()
    x, v = s.sample(x=torch.ones(8, 5), n_steps=0, return_velocity=True)
    assert [name for name, _ in rec.named("ebm_")] == ["ebm_noise_fill_f32"] and torch.equal(x, torch.ones(8, 5)) and v.shape == (8, 5)
