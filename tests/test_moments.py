"""sample_moments and ChainMoments on the CPU: the eager route against the restatement of moments_cases.py on the trajectory
sample() returns, the convergence figures against the closed form of an AR(1) chain, the stuck double well, the edge cases,
and the cases of test_moments_gpu.py themselves (margins, both accept outcomes)."""

import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd.samplers.moments import ChainMoments, RunningMoments, recip_table, split_counted
from moments_cases import HMC_CASES, MARGIN_BAR, hmc_case, two_pass, welford


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------
# the cases the GPU tests run
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim,n,k,burn_in", HMC_CASES)
def test_hmc_cases_meet_the_margin_and_decide_both_ways(kind, dim, n, k, burn_in):
    c = hmc_case(kind, dim, n, k, burn_in)
    assert c["ref64"]["margin"].min().item() > MARGIN_BAR, c["seed"]
    assert torch.equal(c["ref32"]["accepted"], c["ref64"]["accepted"])
    acc = c["ref32"]["accepted"]
    print(kind, dim, "seed", c["seed"], "rejected", int((~acc).sum()), "of", acc.numel())
    if n >= 37:
        assert 0 < acc.sum() < acc.numel()


def test_the_restated_recurrence_is_the_two_pass_moments():
    traj = torch.randn(7, 34, 3, generator=_gen(0), dtype=torch.float64) * 3.0 + 5.0
    mean, m2 = welford(traj, 17, torch.float64, recip=(1.0 / torch.arange(1, 18, dtype=torch.float64)))
    want_mean, want_m2 = two_pass(traj, 17)
    assert torch.allclose(mean, want_mean, rtol=1e-13, atol=0) and torch.allclose(m2, want_m2, rtol=1e-12, atol=0)
    assert torch.equal(recip_table(5), torch.tensor([1.0, 0.5, 1.0 / 3.0, 0.25, 0.2], dtype=torch.float64).float())


# ---------------------------------------------------------------------------------
# the eager route against the restatement
# ---------------------------------------------------------------------------------
def _samplers():
    return {
        "langevin": lambda: ta.LangevinDynamics(ta.DoubleWellModel(barrier_height=2.0), step_size=0.01),
        "langevin_gmm": lambda: ta.LangevinDynamics(ta.core.ring_mixture(4, 3, radius=2.0, sigma=0.7), step_size=0.02, noise_scale=0.8),
        "hmc": lambda: ta.HamiltonianMonteCarlo(ta.DoubleWellModel(barrier_height=2.0), step_size=0.2, n_leapfrog_steps=3),
    }


@pytest.mark.parametrize("which", sorted(_samplers()))
@pytest.mark.parametrize("n_steps,burn_in", [(4, 0), (11, 3), (40, 6)])
def test_eager_route_is_the_recurrence_on_samples_trajectory(which, n_steps, burn_in):
    make = _samplers()[which]
    x0 = torch.randn(13, 3, generator=_gen(1))
    h = (n_steps - burn_in) // 2
    x_final, mom = make().sample_moments(x=x0, n_steps=n_steps, burn_in=burn_in, energy=True, generator=_gen(7))
    s = make()
    traj = s.sample(x=x0, n_steps=n_steps, return_trajectory=True, generator=_gen(7))
    assert torch.equal(x_final, s.sample(x=x0, n_steps=n_steps, generator=_gen(7)))
    assert torch.equal(x_final, traj[:, -1])
    counted = traj[:, burn_in:]
    mean, m2 = welford(counted, h)
    assert torch.equal(mom.chain_mean, mean) and torch.equal(mom.chain_m2, m2)
    e_traj = s.model(counted.reshape(-1, 3)).view(13, 2 * h)
    e_mean, e_m2 = welford(e_traj, h)
    assert torch.equal(mom.energy_mean, e_mean) and torch.equal(mom.energy_m2, e_m2)
    assert mom.half_len == h and mom.n_nonfinite == 0
    if which == "hmc":
        assert mom.acceptance_rate.shape == (n_steps,)
        moved = (traj[:, 1:] != traj[:, :-1]).any(dim=2).float().mean(dim=0)
        assert torch.allclose(mom.acceptance_rate[1:], moved)
    else:
        assert mom.acceptance_rate is None
    # against float64 moments of the same trajectory
    want_mean, want_m2 = two_pass(counted, h)
    assert torch.allclose(mom.chain_mean.double(), want_mean, atol=1e-5) and torch.allclose(mom.chain_m2.double(), want_m2, rtol=1e-3, atol=1e-5)


# ---------------------------------------------------------------------------------
# ChainMoments against the closed form of an AR(1) chain
# ---------------------------------------------------------------------------------
def harmonic_closed_form(h=200):
    """HarmonicModel(k = 4) under Langevin with step 0.05 and noise_coef sqrt(2): x' = 0.8 x + sqrt(0.1) z."""
    rho, eta = 0.8, 0.05
    v = 2.0 * eta / (1.0 - rho**2)
    var_mean = v / h * ((1 + rho) / (1 - rho) - 2 * rho * (1 - rho**h) / (h * (1 - rho) ** 2))
    w = h / (h - 1) * (v - var_mean)
    rhat = math.sqrt((h - 1) / h + var_mean / w)
    return v, var_mean, rhat


def check_harmonic_law(mom, n, h=200):
    """The bars of the closed-form test, shared with the fused route's (test_moments_gpu.py)."""
    v, var_mean, rhat = harmonic_closed_form(h)
    assert abs(rhat - 1.0202) < 1e-4
    M = 2 * n
    bar = 4.5 * math.sqrt(2.0 / (M - 1))
    assert mom.n_nonfinite == 0 and abs(mom.ess_rel_stderr - math.sqrt(2.0 / (M - 1))) < 1e-12
    b_rel = mom.between_var.cpu() / var_mean - 1.0
    ess_ratio = mom.ess.cpu() / (M * v / var_mean)
    print("B/l relative", b_rel.tolist(), "z", (b_rel / math.sqrt(2.0 / (M - 1))).tolist(), "ess ratio", ess_ratio.tolist(),
          "rhat", mom.rhat.tolist())
    assert (b_rel.abs() <= bar).all(), b_rel
    assert ((ess_ratio - 1.0).abs() <= bar).all(), ess_ratio
    assert ((mom.rhat.cpu() - rhat).abs() <= 0.002).all(), mom.rhat
    assert torch.allclose(mom.var.cpu(), torch.full((4,), v, dtype=torch.float64), rtol=0.02)
    assert (mom.mean.cpu().abs() < 5.0 * math.sqrt(var_mean / M)).all()


def test_harmonic_chain_meets_the_closed_form():
    n, h = 4096, 200
    v, _, _ = harmonic_closed_form(h)
    s = ta.LangevinDynamics(ta.HarmonicModel(k=4.0), step_size=0.05, noise_scale=1.0)
    g = _gen(0)
    x0 = math.sqrt(v) * torch.randn(n, 4, generator=g)
    _, mom = s.sample_moments(x=x0, n_steps=2 * h, generator=g)
    assert mom.energy_mean is None
    check_harmonic_law(mom, n, h)


# ---------------------------------------------------------------------------------
# the stuck double well
# ---------------------------------------------------------------------------------
def test_stuck_double_well_raises_the_alarm():
    """Barrier 8, dim 2, step 0.005, 400 steps, half the chains started in each well: no chain crosses, and R-hat says so.
    By the well curvature (E'' = 8 h b^2 = 64, a within-well variance of 1 / 64 against wells at +-1) it is about 8;
    measured on the CPU eager route: 6.57 and 6.76 (the quartic wall widens the well; docs/design/moments.md).  The
    between-sequence ESS of such a run is about M, one draw per sequence: it counts sequences, R-hat is what raises the alarm."""
    n = 512
    x0 = torch.ones(n, 2)
    x0[: n // 2] = -1.0
    make = lambda: ta.LangevinDynamics(ta.DoubleWellModel(barrier_height=8.0), step_size=0.005)  # noqa: E731
    _, mom = make().sample_moments(x=x0, n_steps=400, generator=_gen(3))
    print("stuck double well: rhat", mom.rhat.tolist(), "ess", mom.ess.tolist())
    assert (mom.rhat > 1.1).all()
    assert (mom.rhat > 4.0).all() and (mom.rhat < 16.0).all()
    traj = make().sample(x=x0, n_steps=400, return_trajectory=True, generator=_gen(3))
    mean64, m264 = two_pass(traj, 200)
    want = ChainMoments(mean64, m264, 200)
    assert torch.allclose(mom.rhat, want.rhat, rtol=1e-3, atol=0)
    assert ((mom.ess > 0.9 * 2 * n) & (mom.ess < 1.1 * 2 * n)).all()


# ---------------------------------------------------------------------------------
# edge cases
# ---------------------------------------------------------------------------------
def test_an_odd_count_burns_one_more_step():
    assert split_counted(11, 2) == (3, 4) and split_counted(11, 3) == (3, 4) and split_counted(4, 0) == (0, 2)
    s = ta.LangevinDynamics(ta.DoubleWellModel(), step_size=0.01)
    x0 = torch.randn(5, 2, generator=_gen(2))
    xa, a = s.sample_moments(x=x0, n_steps=11, burn_in=2, generator=_gen(4))
    xb, b = s.sample_moments(x=x0, n_steps=11, burn_in=3, generator=_gen(4))
    assert a.half_len == 4 and torch.equal(xa, xb) and torch.equal(a.chain_mean, b.chain_mean) and torch.equal(a.chain_m2, b.chain_m2)


@pytest.mark.parametrize("n_steps,burn_in", [(3, 0), (2, 0), (5, 2), (4, 5), (4, -1)])
def test_too_few_counted_steps_raise(n_steps, burn_in):
    for s in (ta.LangevinDynamics(ta.DoubleWellModel(), step_size=0.01),
              ta.HamiltonianMonteCarlo(ta.DoubleWellModel(), step_size=0.1, n_leapfrog_steps=2)):
        with pytest.raises(ValueError):
            s.sample_moments(x=torch.zeros(3, 2), n_steps=n_steps, burn_in=burn_in)


def test_a_nan_chain_is_left_out_and_counted():
    s = ta.LangevinDynamics(ta.DoubleWellModel(), step_size=0.01)
    x0 = torch.randn(9, 3, generator=_gen(5))
    bad = x0.clone()
    bad[4, 1] = float("nan")
    _, clean = s.sample_moments(x=x0, n_steps=12, energy=True, generator=_gen(6))
    _, got = s.sample_moments(x=bad, n_steps=12, energy=True, generator=_gen(6))
    others = [i for i in range(9) if i != 4]
    assert got.n_nonfinite == 1 and clean.n_nonfinite == 0
    assert torch.equal(got.chain_mean[:, others], clean.chain_mean[:, others])
    assert torch.equal(got.chain_m2[:, others], clean.chain_m2[:, others])
    assert torch.equal(got.energy_mean[:, others], clean.energy_mean[:, others])
    assert torch.isfinite(got.rhat).all() and torch.isfinite(got.ess).all() and torch.isfinite(got.energy_rhat)
    # the figures are those of the eight clean chains alone
    alone = ChainMoments(clean.chain_mean[:, others], clean.chain_m2[:, others], 6)
    assert torch.equal(got.rhat, alone.rhat) and torch.equal(got.ess, alone.ess) and torch.equal(got.mean, alone.mean)


def test_running_moments_refuses_a_wrong_count():
    acc = RunningMoments(2)
    for _ in range(3):
        acc.add(torch.zeros(2, 2))
    with pytest.raises(ValueError):
        acc.result()
    acc.add(torch.zeros(2, 2))
    assert acc.result().half_len == 2
    with pytest.raises(ValueError):
        acc.add(torch.zeros(2, 2))
