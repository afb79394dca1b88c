"""AnnealedImportanceSampling without a GPU: the eager route against an independent restatement (ais_cases.restate) that
replays the same generator draws, the estimator's formulas on a hand-made weight vector, the class's validation, and the
refusals ebm_ais_chain_f32 makes in front of any launch."""

import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib
from torchebm_amd.samplers.ais import ais_betas, ais_estimate
from ais_cases import energy_spec, f32, linear_betas, model_of, oracle_of, restate, sigmoid_betas


def _replay(seed, n, dim, T, base_std):
    """The draws the eager route takes from a generator seeded with `seed`: randn(n, dim) for the start, then randn(n, dim) and
    rand(n) per step."""
    g = torch.Generator().manual_seed(seed)
    x0 = f32(base_std) * torch.randn(n, dim, generator=g)
    z, u = [], []
    for _ in range(T):
        z.append(torch.randn(n, dim, generator=g))
        u.append(torch.rand(n, generator=g))
    return x0, torch.stack(z), torch.stack(u)


@pytest.mark.parametrize("kind,dim,T,schedule,eps,L,base_std", [
    ("double_well", 3, 7, "linear", 0.25, 3, 1.0),
    ("double_well", 8, 12, "sigmoid", tuple(0.2 - 0.005 * t for t in range(12)), 4, 1.3),  # a step size per transition
    ("harmonic", 5, 9, "sigmoid", 0.6, 5, 0.8),
    ("harmonic", 4, 1, "linear", 0.7, 2, 1.0),                                              # T = 1: the table (0, 1)
])
def test_eager_equals_the_restatement_bit_for_bit(kind, dim, T, schedule, eps, L, base_std):
    spec, n = energy_spec(kind, dim), 64
    x0, z, u = _replay(11, n, dim, T, base_std)
    betas = sigmoid_betas(T) if schedule == "sigmoid" else linear_betas(T)
    table = eps if isinstance(eps, tuple) else (eps,) * T
    want = restate(oracle_of(spec), x0, z, u, betas, table, L, base_std, torch.float32)
    assert T < 3 or (want["accepted"].any() and not want["accepted"].all()), "the case rejects nothing"
    s = ta.AnnealedImportanceSampling(model_of(spec), n_temperatures=T, schedule=schedule, step_size=eps, n_leapfrog_steps=L,
                                      base_std=base_std)
    assert torch.equal(s.betas, betas) and s.n_temperatures == T
    assert s._route(dim)[0] == "eager"  # a CPU instance
    got = s.run(n, dim, generator=torch.Generator().manual_seed(11))
    assert torch.equal(got.samples, want["x"]) and torch.equal(got.log_weights, want["logw"])
    assert torch.equal(got.acceptance_rate, want["accepted"].float().mean(dim=1))
    log_z0 = 0.5 * dim * math.log(2 * math.pi * base_std**2)
    lw = want["logw"].double()
    assert got.log_z == pytest.approx(log_z0 + torch.logsumexp(lw, 0).item() - math.log(n), abs=1e-12)
    assert got.n_nonfinite == 0 and 1.0 <= got.ess <= n
    # betas= gives the same run as the schedule that made them
    again = ta.AnnealedImportanceSampling(model_of(spec), betas=betas.tolist(), step_size=eps, n_leapfrog_steps=L, base_std=base_std)
    assert torch.equal(again.run(n, dim, generator=torch.Generator().manual_seed(11)).log_weights, want["logw"])


def test_the_estimate_follows_its_formulas():
    lw = torch.tensor([0.3, -1.2, 2.0, float("nan"), -0.4, float("-inf"), 1.1], dtype=torch.float64)
    log_z, stderr, ess, bad = ais_estimate(lw, 1.5)
    w = torch.tensor([math.exp(v) for v in (0.3, -1.2, 2.0, -0.4, 1.1)], dtype=torch.float64)  # the NaN and the -inf weigh nothing
    n = 7
    assert bad == 2
    assert log_z == pytest.approx(1.5 + math.log(w.sum().item() / n), abs=1e-12)
    want_ess = w.sum().item() ** 2 / (w * w).sum().item()
    assert ess == pytest.approx(want_ess, rel=1e-12)
    assert stderr == pytest.approx(math.sqrt(1.0 / want_ess - 1.0 / n), rel=1e-12)
    # equal weights: the whole population counts and the estimate has no spread
    log_z, stderr, ess, bad = ais_estimate(torch.full((5,), -2.0), 0.0)
    assert log_z == pytest.approx(-2.0) and ess == pytest.approx(5.0) and stderr == pytest.approx(0.0, abs=1e-7) and bad == 0


def test_log_z_of_a_harmonic_well_on_the_eager_route():
    """Harmonic(k = 4), dim 3: log Z = 1.5 log(2 pi / 4).  256 chains x 16 temperatures on the CPU; the bar is the estimate's own
    standard error, 4.5 of them (the law test of test_ais_gpu.py at a size that takes a fraction of a second here)."""
    s = ta.AnnealedImportanceSampling(ta.HarmonicModel(k=4.0), n_temperatures=16, step_size=0.35, n_leapfrog_steps=3)
    r = s.run(256, 3, generator=torch.Generator().manual_seed(0))
    truth = 1.5 * math.log(2 * math.pi / 4.0)
    print("log_z", r.log_z, "truth", truth, "stderr", r.log_z_stderr, "ess", r.ess, "acceptance", r.acceptance_rate.tolist())
    assert r.ess >= 256 / 8
    assert abs(r.log_z - truth) <= 4.5 * r.log_z_stderr
    data = torch.randn(10, 3, generator=torch.Generator().manual_seed(1))
    ll = s.log_likelihood(data, r)
    assert ll.shape == (10,) and torch.allclose(ll, -ta.HarmonicModel(k=4.0)(data) - r.log_z)


def test_schedules_and_validation():
    for T in (1, 2, 50):
        for schedule in ("linear", "sigmoid"):
            b = ais_betas(T, schedule)
            assert b.dtype == torch.float32 and b.shape == (T + 1,) and b[0] == 0.0 and b[-1] == 1.0 and (b[1:] >= b[:-1]).all()
    assert torch.equal(ais_betas(4, "linear"), torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0]))
    d = ais_betas(50, "sigmoid").diff()
    assert d[0] < d[25] and d[-1] < d[25]  # short steps at both ends
    m = ta.DoubleWellModel()
    with pytest.raises(ValueError, match="n_temperatures"):
        ta.AnnealedImportanceSampling(m, n_temperatures=0)
    with pytest.raises(ValueError, match="schedule"):
        ta.AnnealedImportanceSampling(m, schedule="cosine")
    for betas in [(0.0,), (0.1, 1.0), (0.0, 0.9), (0.0, 0.6, 0.5, 1.0)]:
        with pytest.raises(ValueError, match="betas"):
            ta.AnnealedImportanceSampling(m, betas=betas)
    with pytest.raises(ValueError, match="one value per transition"):
        ta.AnnealedImportanceSampling(m, n_temperatures=4, step_size=(0.1, 0.1))
    with pytest.raises(ValueError, match="step_size must be positive"):
        ta.AnnealedImportanceSampling(m, n_temperatures=2, step_size=(0.1, -0.1))
    with pytest.raises(ValueError, match="n_leapfrog_steps"):
        ta.AnnealedImportanceSampling(m, n_leapfrog_steps=0)
    with pytest.raises(ValueError, match="base_std"):
        ta.AnnealedImportanceSampling(m, base_std=0.0)
    s = ta.AnnealedImportanceSampling(m, n_temperatures=3)
    with pytest.raises(ValueError, match="n_chains and dim"):
        s.run(0, 2)
    assert ta.samplers.AnnealedImportanceSampling is ta.AnnealedImportanceSampling


def test_a_hand_written_energy_runs_on_the_eager_route():
    class Quartic(ta.BaseModel):
        def forward(self, x):
            return (x**4).sum(dim=-1)

    s = ta.AnnealedImportanceSampling(Quartic(), n_temperatures=8, step_size=0.2, n_leapfrog_steps=3)
    r = s.run(64, 2, generator=torch.Generator().manual_seed(2))
    # Z = (2 Gamma(5/4))^2 per pair of coordinates
    truth = 2 * math.log(2 * math.gamma(1.25))
    assert r.samples.shape == (64, 2) and r.log_weights.shape == (64,) and r.acceptance_rate.shape == (8,)
    assert math.isfinite(r.log_z) and abs(r.log_z - truth) <= 4.5 * r.log_z_stderr + 1e-12


def _abi_call(desc, x=16, logw=16, dim=32, T=3, L=2, beta=16, eps=16, x0=None, p=None, u=None):
    _lib.call("ebm_ais_chain_f32", desc, x, logw, 8, dim, T, L, beta, eps, 1.0, 1.0, None, None, x0, p, u, 0, 0, None)


def test_abi_refusals_need_no_gpu():
    """Every refusal comes in front of any launch (the pointers below are never dereferenced)."""
    desc = _lib.EnergyDesc()
    desc.kind = _lib.ENERGY_DOUBLE_WELL
    with pytest.raises(ValueError, match="state pointer is NULL"):
        _abi_call(desc, x=None)
    with pytest.raises(ValueError, match="logw is NULL"):
        _abi_call(desc, logw=None)
    with pytest.raises(ValueError, match="n_temps=0"):
        _abi_call(desc, T=0)
    with pytest.raises(ValueError, match="n_leapfrog=0"):
        _abi_call(desc, L=0)
    with pytest.raises(RuntimeError, match=r"code -3.*dim 257 > 256"):  # EBM_EDIM: one vector per lane
        _abi_call(desc, dim=257)
    with pytest.raises(ValueError, match="beta / eps is NULL"):
        _abi_call(desc, beta=None)
    with pytest.raises(ValueError, match="beta / eps is NULL"):
        _abi_call(desc, eps=None)
    for given in [dict(x0=16), dict(p=16), dict(u=16), dict(x0=16, p=16), dict(x0=16, u=16), dict(p=16, u=16)]:
        with pytest.raises(ValueError, match="must be given together"):  # EBM_EINVAL
            _abi_call(desc, **given)
    desc.kind, desc.dev0 = _lib.ENERGY_MLP, 16
    with pytest.raises(RuntimeError, match=r"code -2.*no annealed-importance-sampling kernel"):  # EBM_EKIND
        _abi_call(desc)
    assert _lib.ABI_VERSION == 9 and "ebm_ais_chain_f32" in _lib.EXPORTS
