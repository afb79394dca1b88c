"""ReplicaExchangeHMC without a GPU: the eager route against an independent restatement (tempering_hmc_cases.restate) that
replays the same generator draws, the sampler's validation and state conventions, and the refusals
ebm_tempering_hmc_chain_f32 makes in front of any launch."""

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib
from tempering_hmc_cases import energy_spec, frozen_case, frozen_masks, model_of, oracle_of, restate, slot_permutation


def _replay(seed, n, R, dim, n_mh, swap_every):
    """The draws the eager route takes from a generator seeded with `seed`: randn(n, R, dim) and rand(n, R) per transition,
    rand(n, R) per event."""
    g = torch.Generator().manual_seed(seed)
    z, ua, us = [], [], []
    for t in range(n_mh):
        z.append(torch.randn(n, R, dim, generator=g))
        ua.append(torch.rand(n, R, generator=g))
        if (t + 1) % swap_every == 0:
            us.append(torch.rand(n, R, generator=g))
    return torch.stack(z), torch.stack(ua), (torch.stack(us) if us else torch.zeros(0, n, R))


def _sampler(spec, temps, swap_every, eps, L):
    return ta.ReplicaExchangeHMC(model_of(spec), step_size=eps, n_leapfrog_steps=L, temperatures=temps, swap_every=swap_every)


@pytest.mark.parametrize("kind,dim,temps,swap_every,n_mh,eps,L", [
    ("double_well", 3, (1.0, 2.0, 4.0), 1, 7, 0.25, 3),                          # one float for every slot
    ("double_well", 8, (1.0, 2.0, 4.0, 8.0), 3, 13, (0.2, 0.18, 0.15, 0.12), 4),  # a step size per slot
    ("harmonic", 5, (1.0, 3.0), 2, 8, (0.6, 0.5), 5),
    ("harmonic", 4, (1.0, 1.5, 2.0, 3.0, 5.0), 1, 6, 0.7, 2),
])
def test_eager_equals_the_restatement_bit_for_bit(kind, dim, temps, swap_every, n_mh, eps, L):
    spec, n, R = energy_spec(kind, dim), 64, len(temps)
    slot_eps = eps if isinstance(eps, tuple) else (eps,) * R
    x0 = torch.randn(n, R, dim, generator=torch.Generator().manual_seed(3))
    z, ua, us = _replay(11, n, R, dim, n_mh, swap_every)
    want = restate(oracle_of(spec), x0, z, ua, us, slot_eps, L, temps, swap_every, torch.float32, thin=2)
    assert want["accepted"].any() and not want["accepted"].all(), "the case rejects nothing"
    assert n_mh // swap_every < 2 or (want["mask"].any() and not want["mask"].all()), "the case swaps nothing"
    s = _sampler(spec, temps, swap_every, eps, L)
    got = s.sample(x=x0, n_steps=n_mh, return_replicas=True, generator=torch.Generator().manual_seed(11))
    assert got.shape == (n, R, dim) and torch.equal(got, want["x"])
    traj = s.sample(x=x0, n_steps=n_mh, thin=2, return_trajectory=True, generator=torch.Generator().manual_seed(11))
    assert torch.equal(traj, want["traj"])
    cold = s.sample(x=x0, n_steps=n_mh, generator=torch.Generator().manual_seed(11))
    assert torch.equal(cold, want["x"][:, 0])


def test_eager_gaussian_matches_the_restatement():
    spec, temps, n, dim, n_mh, eps, L = energy_spec("gaussian", 6), (1.0, 2.0, 4.0), 64, 6, 12, 0.3, 3
    x0 = torch.randn(n, 3, dim, generator=torch.Generator().manual_seed(4))
    for seed in range(12, 40):  # the first seed with no decision within 2e-4 of its threshold (tempering_hmc_cases.case)
        z, ua, us = _replay(seed, n, 3, dim, n_mh, 2)
        want = restate(oracle_of(spec), x0, z, ua, us, (eps,) * 3, L, temps, 2, torch.float32)
        if min(want["mh_margin"].min().item(), want["margin"].min().item()) > 2e-4:
            break
    assert min(want["mh_margin"].min().item(), want["margin"].min().item()) > 2e-4
    assert not want["accepted"].all() and want["mask"].any()
    got = _sampler(spec, temps, 2, eps, L).sample(x=x0, n_steps=n_mh, return_replicas=True, generator=torch.Generator().manual_seed(seed))
    assert (got - want["x"]).abs().max().item() <= 2e-5


@pytest.mark.parametrize("kind,dim,R,n", [("double_well", 5, 3, 37), ("gmm", 32, 4, 37)])
def test_both_ladders_take_the_same_swap_decisions(kind, dim, R, n):
    """States that cannot move (Langevin: eta = 0, zero noise; HMC: eps = 0), the same temperatures and the same u: the two
    restatements decide every swap alike and end with the same permutation of the slots (csrc/ladder.h is one swap event for
    both kernels; test_tempering_hmc_gpu.py holds the kernels to this)."""
    c = frozen_case(kind, dim, R, n)
    lan, hmc = frozen_masks(c)
    assert 0 < int(lan["mask"].sum()) < c["attempts"], "the case needs accepted and rejected swaps"
    assert lan["mask"].shape == (6, n, R - 1) and torch.equal(lan["mask"], hmc["mask"])
    assert hmc["accepted"].all()
    perm = slot_permutation(lan["x"], c["x0"])
    assert torch.equal(perm, slot_permutation(hmc["x"], c["x0"])) and torch.equal(lan["x"], hmc["x"])
    assert (perm != torch.arange(R)).any()


def test_diagnostics_of_the_eager_route():
    spec, temps, n, dim, n_mh, eps, L = energy_spec("double_well", 4), (1.0, 2.0, 4.0), 128, 4, 12, 0.25, 3
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(5))
    z, ua, us = _replay(13, n, 3, dim, n_mh, 2)
    want = restate(oracle_of(spec), x0[:, None].expand(-1, 3, -1), z, ua, us, (eps,) * 3, L, temps, 2, torch.float32, thin=3)
    out, diag = _sampler(spec, temps, 2, eps, L).sample(x=x0, n_steps=n_mh, thin=3, return_trajectory=True, return_diagnostics=True,
                                                         generator=torch.Generator().manual_seed(13))
    assert torch.equal(out, want["traj"]) and out.shape == (n, 4, dim)
    assert diag["mean"].shape == diag["var"].shape == (4, dim) and diag["energy"].shape == (4,)
    assert torch.allclose(diag["mean"], want["traj"].mean(dim=0), atol=1e-6)
    assert torch.allclose(diag["var"], want["traj"].var(dim=0, unbiased=False).clamp(1e-10, 1e10), atol=1e-6)
    e = torch.stack([oracle_of(spec).energy(want["traj"][:, j]).mean() for j in range(4)])
    assert torch.allclose(diag["energy"], e, rtol=1e-5)
    mask = want["mask"]  # [6 events, n, 2]: pair 0 at even events, pair 1 at odd ones
    rate = torch.stack([mask[0::2, :, 0].float().mean(), mask[1::2, :, 1].float().mean()])
    assert diag["swap_acceptance"].shape == (2,) and torch.allclose(diag["swap_acceptance"], rate, atol=1e-6)
    want_rate = want["accepted"].float().mean(dim=(0, 1))  # accepted / proposed per slot over the call
    assert diag["acceptance_rate"].shape == (3,) and torch.allclose(diag["acceptance_rate"], want_rate, atol=1e-6)
    assert (want_rate < 1.0).any() and (want_rate > 0.5).all()


def test_both_starts_and_the_round_trip():
    spec, temps, n, dim, se, eps, L = energy_spec("double_well", 4), (1.0, 2.0, 4.0), 32, 4, 2, 0.25, 3
    s = _sampler(spec, temps, se, eps, L)
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(6))
    # [n, dim]: every slot starts there
    a = s.sample(x=x0, n_steps=8, return_replicas=True, generator=torch.Generator().manual_seed(14))
    b = s.sample(x=x0[:, None].expand(-1, 3, -1).contiguous(), n_steps=8, return_replicas=True, generator=torch.Generator().manual_seed(14))
    assert a.shape == (n, 3, dim) and torch.equal(a, b)
    # two calls of k == one call of 2k when k is an even multiple of swap_every (the event parity continues), on the
    # restatement's draws
    k = 4 * se
    z, ua, us = _replay(15, n, 3, dim, 2 * k, se)
    want = restate(oracle_of(spec), x0[:, None].expand(-1, 3, -1), z, ua, us, (eps,) * 3, L, temps, se, torch.float32)
    g = torch.Generator().manual_seed(15)
    half = s.sample(x=x0, n_steps=k, return_replicas=True, generator=g)
    both = s.sample(x=half, n_steps=k, return_replicas=True, generator=g)
    whole = s.sample(x=x0, n_steps=2 * k, return_replicas=True, generator=torch.Generator().manual_seed(15))
    assert torch.equal(both, whole) and torch.equal(whole, want["x"])
    # x = None draws the start; the input is never modified
    keep = x0.clone()
    out = s.sample(dim=dim, n_samples=5, n_steps=3, generator=torch.Generator().manual_seed(1))
    assert out.shape == (5, dim) and torch.equal(x0, keep)


def test_a_hand_written_energy_runs_on_the_eager_route():
    class Quartic(ta.BaseModel):
        def forward(self, x):
            return (x**4).sum(dim=-1)

    s = ta.ReplicaExchangeHMC(Quartic(), step_size=(0.2, 0.1), n_leapfrog_steps=3, temperatures=(1.0, 3.0), swap_every=2)
    out, diag = s.sample(dim=3, n_samples=16, n_steps=6, return_diagnostics=True, generator=torch.Generator().manual_seed(2))
    assert out.shape == (16, 3) and torch.isfinite(out).all() and 0.0 <= diag["swap_acceptance"][0] <= 1.0
    assert diag["acceptance_rate"].shape == (2,) and ((diag["acceptance_rate"] > 0) & (diag["acceptance_rate"] <= 1)).all()


def test_validation():
    m = ta.DoubleWellModel()
    for temps in [(1.0,), (), (1.0, 1.0), (2.0, 1.0), (0.0, 1.0), (-1.0, 2.0)]:
        with pytest.raises(ValueError, match="temperatures"):
            ta.ReplicaExchangeHMC(m, temperatures=temps)
    with pytest.raises(ValueError, match="swap_every"):
        ta.ReplicaExchangeHMC(m, swap_every=0)
    with pytest.raises(ValueError, match="step_size"):
        ta.ReplicaExchangeHMC(m, step_size=0.0)
    with pytest.raises(ValueError, match="one value per slot"):
        ta.ReplicaExchangeHMC(m, step_size=(0.1, 0.1))
    with pytest.raises(ValueError, match="step_size must be positive"):
        ta.ReplicaExchangeHMC(m, step_size=(0.1, 0.1, -0.1, 0.1))
    with pytest.raises(ValueError, match="n_leapfrog_steps"):
        ta.ReplicaExchangeHMC(m, n_leapfrog_steps=0)
    s = ta.ReplicaExchangeHMC(m)
    with pytest.raises(ValueError, match="thin"):
        s.sample(dim=2, thin=0)
    with pytest.raises(ValueError, match="dim must be provided"):
        s.sample()
    with pytest.raises(ValueError, match=r"\[n, dim\] or \[n, 4, dim\]"):
        s.sample(x=torch.zeros(3, 2, 5))
    with pytest.raises(ValueError, match="exclude each other"):
        s.sample(dim=2, return_trajectory=True, return_replicas=True)
    assert ta.samplers.ReplicaExchangeHMC is ta.ReplicaExchangeHMC and s.n_replicas == 4 and s.swap_every == 1
    assert s._route(torch.zeros(2, 4, 8))[0] == "eager"  # a CPU state


def _abi_call(desc, x=16, R=4, dim=32, n_mh=3, L=2, swap_every=1, thin=1, eps=16, sqrt_temp=16, beta=16, p=None, ua=None, us=None):
    _lib.call("ebm_tempering_hmc_chain_f32", desc, x, 8, R, dim, n_mh, L, eps, sqrt_temp, beta, swap_every, thin, None, None, None,
              None, p, ua, us, 0, 0, None)


def test_abi_refusals_need_no_gpu():
    """Every refusal comes in front of any launch (the pointers below are never dereferenced)."""
    desc = _lib.EnergyDesc()
    desc.kind = _lib.ENERGY_DOUBLE_WELL
    with pytest.raises(ValueError, match="state pointer is NULL"):
        _abi_call(desc, x=None)
    with pytest.raises(ValueError, match="n_replicas=1"):
        _abi_call(desc, R=1)
    with pytest.raises(ValueError, match="n_replicas=65"):
        _abi_call(desc, R=65, dim=2)
    with pytest.raises(RuntimeError, match=r"code -3.*dim 257 > 256"):   # EBM_EDIM: one vector per lane
        _abi_call(desc, R=2, dim=257)
    with pytest.raises(RuntimeError, match=r"code -3.*does not fit one workgroup"):
        _abi_call(desc, R=5, dim=256)   # 64 lanes per replica
    with pytest.raises(RuntimeError, match=r"code -3.*does not fit one workgroup"):
        _abi_call(desc, R=64, dim=32)   # 8 lanes per replica
    with pytest.raises(ValueError, match="swap_every=0"):
        _abi_call(desc, swap_every=0)
    with pytest.raises(ValueError, match="thin=0"):
        _abi_call(desc, thin=0)
    with pytest.raises(ValueError, match="n_leapfrog=0"):
        _abi_call(desc, L=0)
    with pytest.raises(ValueError, match="eps / sqrt_temp / beta is NULL"):
        _abi_call(desc, beta=None)
    for given in [dict(p=16), dict(ua=16), dict(us=16), dict(p=16, ua=16), dict(p=16, us=16), dict(ua=16, us=16)]:
        with pytest.raises(ValueError, match="must be given together"):
            _abi_call(desc, **given)
    desc.kind, desc.dev0 = _lib.ENERGY_MLP, 16
    with pytest.raises(RuntimeError, match=r"code -2.*no replica-exchange kernel"):  # EBM_EKIND
        _abi_call(desc)
    assert _lib.ABI_VERSION == 9 and "ebm_tempering_hmc_chain_f32" in _lib.EXPORTS
