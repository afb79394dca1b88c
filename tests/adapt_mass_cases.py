"""Dual-averaging step-size adaptation under a scalar or diagonal mass (include/ebm_hip_adapt_mass.h,
ebm_ghmc_adapt_chain_mass_f32): an independent restatement of the massed adapting recurrence in torch ops on the oracle energies
-- mass_cases.restate_ghmc's transition with the step size, the refresh constants, the drift and the three controller values held
per chain -- the cases the tests run, and their inputs.  Shared by test_adapt_mass.py (CPU tier) and test_adapt_mass_gpu.py; it
never calls the package."""

import functools
import math

import torch

from adapt_cases import BOUNDS, DELTA, LAW, LAW_SIGMAS, MU_FACTOR, f32, pooled_log, table  # noqa: F401  (re-exported for the tests)
from ghmc_cases import MARGIN_BAR
from mass_cases import (GAMMA, GHMC_CASES, TEMP, _force, _hamiltonian, energy_spec, forms, ghmc_inputs, ghmc_step, mass_of,  # noqa: F401
                        model_of, oracle_of)

SEED_CAP = 200  # seeds tried per case, the cap adapt_cases uses


def restate(energy, x0, p0, z, u, eps0, n_leapfrog, gamma, temp, mass, dtype=torch.float32, thin=1, xi0=None, n_adapt=None, m0=0,
            delta=DELTA, mu_factor=MU_FACTOR, mu=None, bounds=BOUNDS, da=None, close=True):
    """adapt_cases.restate with a mass: x0, p0 [n, dim] (p0 None: (sqrt_temp m_sqrt) xi0), z [n_mh, n, dim], u [n_mh, n] -> x, v
    (the momentum), traj, accepted, margin, da [3, n], eps_trace [n_mh, n], alpha_mean [n], alphas [n_mh, n].  Every operation
    rounded on its own in `dtype`; float64 runs the same fp32 constants, mass forms and table, upcast."""
    n_mh, n = z.shape[0], x0.shape[0]
    n_adapt = n_mh if n_adapt is None else n_adapt
    full = math.isinf(gamma)
    gamma_l = 0.0 if full else f32(gamma * n_leapfrog)
    temp32, sqrt_temp, beta = f32(temp), f32(math.sqrt(temp)), f32(1.0 / temp)
    delta32 = f32(delta)
    mu32 = f32(math.log(mu_factor * eps0) if mu is None else mu)
    log_min, log_max = f32(math.log(bounds[0])), f32(math.log(bounds[1]))
    tab = table(n_adapt, m0).tolist()
    scalar = isinstance(mass, float)
    m_raw, m_sqrt, m_safe = forms(mass, dtype)
    x = x0.to(dtype).clone()
    p = ((sqrt_temp * m_sqrt) * xi0.to(dtype)) if p0 is None else p0.to(dtype).clone()
    if da is None:
        eps, hbar, lbar = torch.full((n,), f32(eps0), dtype=dtype), torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype)
    else:
        eps, hbar, lbar = (row.to(dtype).clone() for row in da)
    accepted, margins, kept, trace, alphas = [], [], [], [], []
    alpha_sum = torch.zeros(n, dtype=dtype)
    for t in range(n_mh):
        trace.append(eps.clone())
        e = eps[:, None]
        if full:
            c1, c2 = 0.0, torch.full((n, 1), sqrt_temp, dtype=dtype)
        else:
            span = gamma_l * eps
            c1 = torch.exp(-span)[:, None]
            c2 = torch.sqrt(temp32 * (-torch.expm1(-2.0 * span)))[:, None]
        refresh = c2 * m_sqrt  # [n, dim] (a scalar mass: [n, 1])
        drift = e / m_safe  # a tensor division: eps / m_safe, IEEE, per chain and coordinate
        p = c1 * p + refresh * z[t].to(dtype)  # O
        h0 = _hamiltonian(energy.energy(x), p, m_raw, scalar)
        xp, w = x, p
        for _ in range(n_leapfrog):  # the safe-mode leapfrog sequence with the drift drift_j p_j, the chain's own step size
            w_half = w + 0.5 * e * _force(energy, xp)
            xp = xp + drift * w_half
            w = w_half + 0.5 * e * _force(energy, xp)
            xp = xp.nan_to_num_(nan=0.0)
            w = w.nan_to_num_(nan=0.0)
        h1 = _hamiltonian(energy.energy(xp), w, m_raw, scalar)
        a = torch.exp((beta * (h0 - h1)).clamp_(min=-50.0, max=50.0)).clamp_(max=1.0)
        ut = u[t].to(dtype)
        acc = ut < a
        accepted.append(acc)
        margins.append(torch.where(a == a, (ut - a).abs().double(), torch.full((), float("inf"), dtype=torch.float64)))
        x = torch.where(acc[:, None], xp, x)
        p = torch.where(acc[:, None], w, -p)  # the flip: the negative of the momentum after O
        al = torch.where(a == a, a, torch.zeros_like(a))  # NaN counts as 0
        alphas.append(al)
        if t < n_adapt:
            alpha_sum = alpha_sum + al
            hbar = tab[t][0] * hbar + tab[t][1] * (delta32 - al)
            le = (mu32 - tab[t][2] * hbar).clamp(min=log_min, max=log_max)
            lbar = tab[t][3] * le + tab[t][4] * lbar
            eps = torch.exp(lbar) if (close and t + 1 == n_adapt) else torch.exp(le)
        if (t + 1) % thin == 0:
            kept.append(x.clone())
    dim = x0.shape[1]
    return {"x": x, "v": p, "traj": torch.stack(kept, dim=1) if kept else torch.zeros(n, 0, dim, dtype=dtype),
            "accepted": torch.stack(accepted), "margin": min((m.min().item() for m in margins), default=float("inf")),
            "da": torch.stack((eps, hbar, lbar)), "eps_trace": torch.stack(trace), "alphas": torch.stack(alphas),
            "alpha_mean": alpha_sum / n_adapt if n_adapt > 0 else alpha_sum}


# mass_cases' 20 generalized-HMC cases (kind, dim, n, thin, L, mass form) x n_mh in {2, 4}; thin 3 becomes 2 so that it divides
CASES = [(kind, dim, n, n_mh, min(thin, 2), L, form) for kind, dim, n, _, thin, L, form in GHMC_CASES for n_mh in (2, 4)]
KINDS = sorted({c[0] for c in CASES})


@functools.lru_cache(maxsize=None)
def case(kind, dim, n, n_mh, thin, L, form, gamma=GAMMA, temp=TEMP):
    """Inputs and both restatements of a case, computed once per session and shared (read-only): ghmc_cases.case's rule -- the seed
    is the first whose fp64 restatement has no decision closer than MARGIN_BAR to its threshold and whose fp32 restatement decides
    alike.  `found` says whether one of the SEED_CAP did; `seed` + 1 is the number of tries."""
    from helpers import to64

    spec, mass = energy_spec(kind, dim), mass_of(form, dim)
    eps0 = ghmc_step(kind, dim, mass)
    found = False
    for seed in range(SEED_CAP):
        x0, p0, z, u = ghmc_inputs(7500 + seed, kind, n, dim, n_mh, mass)
        ref64 = restate(to64(oracle_of(spec)), x0, p0, z, u, eps0, L, gamma, temp, mass, torch.float64, thin)
        if ref64["margin"] <= MARGIN_BAR:
            continue
        ref32 = restate(oracle_of(spec), x0, p0, z, u, eps0, L, gamma, temp, mass, torch.float32, thin)
        if torch.equal(ref32["accepted"], ref64["accepted"]):
            found = True
            break
    return {"spec": spec, "mass": mass, "x0": x0, "v0": p0, "z": z, "u": u, "eps0": eps0, "L": L, "gamma": gamma, "temp": temp,
            "ref32": ref32, "ref64": ref64, "seed": seed, "found": found, "shape": (n, dim), "n_mh": n_mh, "thin": thin,
            "mu": math.log(MU_FACTOR * eps0)}


# ---- the payoff: warmup() on the badly scaled Gaussian of mass_cases (sigma = (1, 0.1, 0.01)), started from the target law
PAYOFF_SIGMAS = 4.5  # the factor of the project's law tests


def payoff_expectation(sigma, n):
    """m_j sigma_j^2 of the regularised estimate in expectation: sigma_j^2 / (N/(N+5) sigma_j^2 + 1e-3 * 5/(N+5))."""
    s2 = torch.tensor(sigma, dtype=torch.float64) ** 2
    return s2 / (n / (n + 5.0) * s2 + 1e-3 * 5.0 / (n + 5.0))


def payoff_margin(n):
    """exp(4.5 sqrt(2 / (N - 1))): the sampling error of a Gaussian sample variance (relative standard error sqrt(2 / (N - 1)))
    at 4.5 standard errors, as a factor."""
    return math.exp(PAYOFF_SIGMAS * math.sqrt(2.0 / (n - 1)))
