"""ebm_tempering_mlp_chain_f32 and the ``fused_mlp_ladder`` opt-in of ReplicaExchangeLangevin without a GPU: the export and its
declaration, the refusals the entry makes in front of any device access, the opt-in's default and CPU behaviour, the one launch of
the opted-in route against a recording stand-in of the library, the calls that stay eager, the conditions every GPU case must
meet and the fp32 restatement of every case against fp64."""

import os
import re

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import fused_cpu  # noqa: F401
from tempering_mlp_cases import (CASES, MARGIN_BAR, MAX_SEEDS, MIN_DECISIONS, case, closest_call, frozen_case, restatement_errors,
                                 swap_attempts, tail_case)

ENTRY = "ebm_tempering_mlp_chain_f32"
ANALYTIC = "ebm_tempering_chain_f32"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ebm_hip.h")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _parameter_list(text, name, prefix=r"EBM_API\s+int\s+"):
    """The parameter list of `name`'s declaration, white space collapsed."""
    m = re.search(prefix + name + r"\s*\(([^)]*)\)", text)
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_the_entry_is_exported_and_declared():
    assert ENTRY in _lib.EXPORTS and ENTRY in _lib._PROTOTYPES
    assert _lib._PROTOTYPES[ENTRY] == _lib._PROTOTYPES[ANALYTIC]  # the same parameter list
    with open(HEADER) as fh:
        header = fh.read()
    assert _parameter_list(header, ENTRY) == _parameter_list(header, ANALYTIC)
    assert len(_parameter_list(header, ENTRY).split(",")) == 19
    assert _lib.ABI_VERSION == 9
    assert hasattr(_lib.lib(), ENTRY)


def _mlp_desc(hidden):
    desc = _lib.EnergyDesc()
    desc.kind, desc.n_comp, desc.dev0 = _lib.ENERGY_MLP, hidden, 16
    return desc


def _abi_call(desc, *, entry=ENTRY, x=16, n=4, R=4, dim=8, k=3, eta=0.05, sqrt_eta=0.05**0.5, coef=16, beta=16, swap_every=1, thin=1,
              traj=None, noise=None, u=None):
    _lib.call(entry, desc, x, n, R, dim, k, eta, sqrt_eta, coef, beta, swap_every, thin, traj, None, noise, u, 0, 0, None)


EINVAL = [
    (dict(x=None), "state pointer is NULL"),
    (dict(coef=None), "noise_coef / beta is NULL"),
    (dict(beta=None), "noise_coef / beta is NULL"),
    (dict(k=0), "k_steps=0"),
    (dict(k=-1), "k_steps=-1"),
    (dict(thin=0), "thin=0"),
    (dict(swap_every=0), "swap_every=0"),
    (dict(noise=16), "must be given together"),
    (dict(u=16), "must be given together"),
    (dict(eta=float("nan")), "both must be finite"),
    (dict(eta=float("inf")), "both must be finite"),
    (dict(sqrt_eta=float("nan")), "both must be finite"),
    (dict(sqrt_eta=-float("inf")), "both must be finite"),
    (dict(x=20), "16-byte aligned"),
    (dict(traj=24), "16-byte aligned"),
    (dict(noise=8, u=16), "16-byte aligned"),
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
        with pytest.raises(RuntimeError, match=r"code -3.*hidden width 64 or 128.*got 96, 8, 4"):  # EBM_EDIM
            _abi_call(_mlp_desc(96), n=n)
        with pytest.raises(RuntimeError, match=r"code -3.*got 256, 8, 4"):
            _abi_call(_mlp_desc(256), n=n)
        with pytest.raises(RuntimeError, match=r"code -3.*1 <= dim <= 128.*got 64, 129, 4"):
            _abi_call(desc, n=n, dim=129)
        with pytest.raises(RuntimeError, match=r"code -3.*got 128, 0, 4"):
            _abi_call(_mlp_desc(128), n=n, dim=0)
        for R in (0, 1, 3, 5, 6, 12, 24, 33, 64):
            with pytest.raises(RuntimeError, match=rf"code -3.*2, 4, 8, 16 or 32 replicas.*got 64, 8, {R}\)"):
                _abi_call(desc, n=n, R=R)
    with pytest.raises(ValueError, match="bad shape"):
        _abi_call(desc, n=-1)
    for R in (2, 4, 8, 16, 32):  # an empty call returns in front of any launch
        _abi_call(desc, n=0, R=R)
    _abi_call(_mlp_desc(128), n=0, dim=128, k=7, thin=3, swap_every=4, noise=16, u=16, traj=32, eta=0.0, sqrt_eta=0.0)
    # ebm_tempering_chain_f32 is untouched: it still refuses the MLP
    with pytest.raises(RuntimeError, match=r"code -2.*no replica-exchange kernel"):
        _abi_call(desc, entry=ANALYTIC)


def test_the_opt_in_is_off_by_default_and_changes_nothing_on_the_cpu():
    assert ta.ReplicaExchangeLangevin.fused_mlp_ladder is False
    assert not hasattr(ta.ReplicaExchangeLangevin, "fused_mlp")  # (the HMC ladder's switch, pinned by its own tests)
    torch.manual_seed(4)
    model = ta.MLPEnergy(4, 64)
    kw = dict(step_size=0.05, noise_scale=1.0, temperatures=(1.0, 2.0, 4.0, 8.0), swap_every=2)
    plain, opted = ta.ReplicaExchangeLangevin(model, **kw), ta.ReplicaExchangeLangevin(model, **kw)
    assert plain.fused_mlp_ladder is False
    opted.fused_mlp_ladder = True
    x0 = torch.randn(48, 4, generator=_gen(1))
    ladders = x0.unsqueeze(1).expand(-1, 4, -1).contiguous()
    assert plain._route(ladders) == ("eager", None) and opted._route(ladders) == ("eager", None)  # CPU states
    a = plain.sample(x=x0, n_steps=7, thin=2, return_trajectory=True, return_diagnostics=True, generator=_gen(9))
    b = opted.sample(x=x0, n_steps=7, thin=2, return_trajectory=True, return_diagnostics=True, generator=_gen(9))
    assert torch.equal(a[0], b[0]) and a[0].shape == (48, 3, 4) and torch.isfinite(a[0]).all()
    for key in ("mean", "var", "energy", "swap_acceptance"):
        assert torch.equal(a[1][key], b[1][key]), key
    ra = plain.sample(x=x0, n_steps=5, return_replicas=True, generator=_gen(9))
    rb = opted.sample(x=x0, n_steps=5, return_replicas=True, generator=_gen(9))
    assert torch.equal(ra, rb) and ra.shape == (48, 4, 4)


def _mlp_sampler(monkeypatch, in_dim=5, hidden=64, temps=(1.0, 2.0, 4.0, 8.0), patch_route=True, **kw):
    model = ta.MLPEnergy(in_dim, hidden)
    s = ta.ReplicaExchangeLangevin(model, temperatures=temps, device="cpu", **kw)
    s.fused_mlp_ladder = True
    spec = ta.core.energies.FusedSpec(_lib.ENERGY_MLP, n_comp=hidden, dev0=model._packed_parameters(), langevin_only=True, dim=in_dim,
                                      hmc=True)
    if patch_route:
        monkeypatch.setattr(s, "_route", lambda x: ("fused_mlp", spec))
    return s, spec


def test_the_opted_in_route_is_one_launch_of_the_entry(fused_cpu, monkeypatch):  # noqa: F811
    _, rec, clones = fused_cpu
    torch.manual_seed(8)
    s, _ = _mlp_sampler(monkeypatch, step_size=0.04, noise_scale=1.5, swap_every=2)
    n, R, dim, k, thin = 37, 4, 5, 11, 3
    x0 = torch.randn(n, dim, generator=_gen(1))
    x_before = x0.clone()
    clones.clear()
    out = s.sample(x=x0, n_steps=k, thin=thin, return_replicas=True, generator=_gen(3))
    calls = rec.named("ebm_")
    assert [name for name, _ in calls] == [ENTRY]
    args = calls[0][1]
    assert out.shape == (n, R, dim) and out.data_ptr() == args[1] and out.data_ptr() != x0.data_ptr() and len(clones) >= 1
    # (energy, x, n_ladders, R, dim, k_steps, eta, sqrt_eta, noise_coef, beta, swap_every, thin, traj, swap_counts, noise, u, seed,
    #  step0, stream)
    assert tuple(args[2:6]) == (n, R, dim, k) and args[6] == 0.04 and args[7] == 0.04**0.5
    assert all(a is not None for a in args[8:10])
    assert tuple(args[10:]) == (2, thin, None, None, None, None, 7, 11, None)
    assert torch.equal(x0, x_before)
    # the ladder's two arrays are ladder_coefficients at the noise scale
    coef, beta = ta.samplers.tempering.ladder_coefficients(1.5, s.temperatures)
    held_coef, held_beta = s._ladder_on(torch.device("cpu"), 1.5)
    assert torch.equal(held_coef, coef) and torch.equal(held_beta, beta) and (args[8], args[9]) == (held_coef.data_ptr(), held_beta.data_ptr())
    # a ladder start is cloned, never written
    rec.calls.clear()
    start = out.clone()
    clones.clear()
    s.sample(x=start, n_steps=k, return_replicas=True, generator=_gen(3))
    (name, args), = rec.named("ebm_")
    assert name == ENTRY and args[1] != start.data_ptr() and start.data_ptr() in clones
    # trajectory and diagnostics: the kept slot-0 states' buffer and the counters; their statistics are torch ops: no further entry
    rec.calls.clear()
    traj, diag = s.sample(x=x0, n_steps=k, thin=thin, return_trajectory=True, return_diagnostics=True, generator=_gen(3))
    (name, args), = rec.named("ebm_")
    assert name == ENTRY and args[12] == traj.data_ptr() and traj.shape == (n, k // thin, dim)
    assert args[13] is not None and args[14:16] == (None, None)
    assert sorted(diag) == ["energy", "mean", "swap_acceptance", "var"] and diag["swap_acceptance"].shape == (R - 1,)
    assert diag["energy"].shape == (k // thin,) and diag["mean"].shape == diag["var"].shape == (k // thin, dim)
    assert torch.equal(x0, x_before)


def test_the_opted_in_route_reserves_two_steps_per_step(fused_cpu, monkeypatch):  # noqa: F811
    _, rec, _ = fused_cpu
    s, _ = _mlp_sampler(monkeypatch, step_size=0.2)
    reserved = []
    monkeypatch.setattr(_rng, "reserve", lambda generator, device, n_steps: reserved.append(n_steps) or (7, 11))
    s.sample(x=torch.zeros(8, 5), n_steps=9)
    assert reserved == [2 * 9] and [name for name, _ in rec.named("ebm_")] == [ENTRY]
    # no step, or no ladder: nothing is launched
    rec.calls.clear()
    out = s.sample(x=torch.ones(8, 5), n_steps=0, return_replicas=True)
    assert reserved == [18, 0] and rec.named("ebm_") == [] and torch.equal(out, torch.ones(8, 4, 5))
    out = s.sample(x=torch.ones(0, 5), n_steps=4)
    assert rec.named("ebm_") == [] and out.shape == (0, 5)


class _CudaLike:
    """What _route reads of a state, for a CUDA fp32 tensor of the given shape (no GPU here)."""

    is_cuda, dtype, ndim = True, torch.float32, 3

    def __init__(self, *shape):
        self.shape = torch.Size(shape)

    def view(self, *shape):
        n = 1
        for s in self.shape:
            n *= s
        return _CudaLike(n // shape[-1], shape[-1])


def test_which_calls_stay_eager(monkeypatch):
    """_route on a stand-in for a CUDA fp32 state: the opt-in, the ladder lengths, the widths and the schedulers decide."""
    import torchebm_amd.samplers.tempering as tempering

    def route(s, n=6, dim=5):
        return s._route(_CudaLike(n, s.n_replicas, dim))[0]

    def with_spec(s, spec):
        monkeypatch.setattr(tempering, "fused_spec_for", lambda model, rows, kw: spec)
        return s

    s, spec = _mlp_sampler(monkeypatch, patch_route=False, step_size=0.2)
    with_spec(s, spec)
    assert s._route(_CudaLike(6, 4, 5)) == ("fused_mlp", spec)
    s.fused_mlp_ladder = False
    assert s._route(_CudaLike(6, 4, 5)) == ("eager", None)  # no opt-in: what the MLP got before the route existed
    s.fused_mlp_ladder = True
    assert route(s, dim=6) == "eager"  # dim != in_dim
    for R in (2, 4, 8, 16, 32):
        t, sp = _mlp_sampler(monkeypatch, patch_route=False, temps=tuple(1.0 + r for r in range(R)), step_size=0.2)
        assert route(with_spec(t, sp)) == "fused_mlp", R
    for R in (3, 5, 6, 12, 33, 64):
        t, sp = _mlp_sampler(monkeypatch, patch_route=False, temps=tuple(1.0 + r for r in range(R)), step_size=0.2)
        assert route(with_spec(t, sp)) == "eager", R
    t, sp = _mlp_sampler(monkeypatch, patch_route=False, step_size=ta.core.schedules.LinearScheduler(0.3, 0.1, 10))
    assert route(with_spec(t, sp)) == "eager"  # a scheduled step size
    t, sp = _mlp_sampler(monkeypatch, patch_route=False, step_size=0.2, noise_scale=ta.core.schedules.LinearScheduler(1.0, 0.5, 10))
    assert route(with_spec(t, sp)) == "eager"  # a scheduled noise scale
    t, sp = _mlp_sampler(monkeypatch, patch_route=False, hidden=32, step_size=0.2)
    assert route(with_spec(t, sp)) == "eager"  # a width without kernels
    t, sp = _mlp_sampler(monkeypatch, patch_route=False, in_dim=128, hidden=128, step_size=0.2)
    assert route(with_spec(t, sp), dim=128) == "fused_mlp"
    with_spec(t, None)
    assert route(t, dim=128) == "eager"  # a model without a fused spec
    # an analytic energy keeps its own one-launch route with the opt-in set
    well = ta.ReplicaExchangeLangevin(ta.DoubleWellModel(), step_size=0.1)
    well.fused_mlp_ladder = True
    assert route(with_spec(well, ta.DoubleWellModel().fused_spec())) == "fused"
    # and on the CPU everything is eager
    assert s._route(torch.zeros(6, 4, 5))[0] == "eager"


@pytest.mark.parametrize("in_dim,hidden,R,n,swap_every,k", CASES)
def test_every_case_decides_clearly_both_ways_and_its_fp32_restatement_tracks_fp64(in_dim, hidden, R, n, swap_every, k):
    """The conditions of the GPU cases: a seed among the first MAX_SEEDS whose fp64 restatement has no swap decision within
    MARGIN_BAR of its threshold, whose fp32 restatement decides alike and which holds at least MIN_DECISIONS accepted and as many
    rejected swaps; and ladders that do not diverge -- the fp32 restatement's max error against fp64 is at most 1e-4 x max |ref|
    for the slot matrix and the kept slot-0 states, so '4 x the fp32 restatement's own error' is a bar on round-off, not on
    chaos."""
    c = case(in_dim, hidden, R, n, swap_every, k)
    mask = c["ref64"]["mask"]
    tried = int(swap_attempts(k // swap_every, n, R).sum())
    took = int(mask.sum())
    print(f"dim {in_dim} H {hidden} R {R} n {n} swap_every {swap_every} k {k}: seed {c['seed']}, margin "
          f"{closest_call(c['ref64']):.2e}, swaps {took} of {tried}")
    assert c["found"] and c["seed"] < MAX_SEEDS
    assert closest_call(c["ref64"]) > MARGIN_BAR
    assert torch.equal(c["ref32"]["mask"], mask)
    assert mask.shape == (k // swap_every, n, R - 1) and took >= MIN_DECISIONS and tried - took >= MIN_DECISIONS
    assert c["ref64"]["traj"].shape == (n, k // c["thin"], in_dim)
    for key, (err, scale) in restatement_errors(c).items():
        print(f"    {key} fp32 err {err:.3e} max|ref| {scale:.3e}")
        assert err <= 1e-4 * scale, (key, err, scale)


@pytest.mark.parametrize("in_dim,hidden,R,n", [(5, 64, 4, 10), (64, 128, 8, 5)])
def test_the_case_with_a_kept_last_step_and_no_event_behind_it_meets_the_conditions(in_dim, hidden, R, n):
    c = tail_case(in_dim, hidden, R, n)
    assert c["found"] and closest_call(c["ref64"]) > MARGIN_BAR and torch.equal(c["ref32"]["mask"], c["ref64"]["mask"])
    assert c["ref64"]["mask"].shape == (1, n, R - 1) and c["ref64"]["traj"].shape == (n, 2, in_dim)
    for key, (err, scale) in restatement_errors(c).items():
        assert err <= 1e-4 * scale, (key, err, scale)


def test_the_frozen_case_swaps_both_ways():
    c = frozen_case(5, 64, 4, 19)
    assert c["found"] and 0 < int(c["ref64"]["mask"].sum()) < int(swap_attempts(6, 19, 4).sum())
    assert torch.equal(c["ref64"]["x"].float().sort(dim=1).values, c["x0"].sort(dim=1).values)  # nothing moved but by a swap
