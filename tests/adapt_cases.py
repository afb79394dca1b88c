"""Dual-averaging step-size adaptation (include/ebm_hip_adapt.h, ebm_ghmc_adapt_chain_f32): an independent restatement of the
recurrence in torch ops on the oracle energies -- ghmc_cases.restate's transition with the step size, the refresh constants and
the three controller values held per chain -- the cases the tests run, and their inputs.  Shared by test_adapt.py (CPU tier)
and test_adapt_gpu.py; it never calls the package."""

import functools
import math

import torch

from ghmc_cases import (CASES as GHMC_CASES, GAMMA, MARGIN_BAR, TEMP, _force, _hamiltonian, draw_inputs, energy_spec,  # noqa: F401
                        model_of, oracle_of, step_size)

# Stan's dual-averaging constants, and the target
T0, GAMMA_DA, KAPPA, MU_FACTOR, DELTA = 10.0, 0.05, 0.75, 10.0, 0.8
BOUNDS = (1e-6, 1e3)


def f32(value):
    """A double rounded once to fp32, as the Python float of that fp32 value."""
    return torch.tensor(value, dtype=torch.float64).to(torch.float32).item()


def table(n_adapt, m0=0, t0=T0, gamma_da=GAMMA_DA, kappa=KAPPA):
    """Row t = (1 - w, w, s, k, 1 - k), m = m0 + t + 1: plain double arithmetic value by value, each rounded once."""
    rows = []
    for t in range(n_adapt):
        m = float(m0 + t + 1)
        w, k = 1.0 / (m + t0), m ** (-kappa)
        rows.append([f32(1.0 - w), f32(w), f32(math.sqrt(m) / gamma_da), f32(k), f32(1.0 - k)])
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32).reshape(n_adapt, 5)


def restate(energy, x0, v0, z, u, eps0, n_leapfrog, gamma, temp, dtype=torch.float32, thin=1, xi0=None, n_adapt=None, m0=0,
            delta=DELTA, mu_factor=MU_FACTOR, mu=None, bounds=BOUNDS, da=None, close=True):
    """ghmc_cases.restate with the controller: x0 [n, dim], v0 [n, dim] (or None: sqrt_temp * xi0), z [n_mh, n, dim], u [n_mh, n]
    -> x, v, traj, accepted, margin as there, and da [3, n], eps_trace [n_mh, n], alpha_mean [n], alphas [n_mh, n].  Every
    operation rounded on its own in `dtype`; float64 runs the same fp32 constants and table, upcast.  `da` continues an earlier
    call's controllers; close=False keeps the last iterate at the end of the adaptation."""
    n_mh, n = z.shape[0], x0.shape[0]
    n_adapt = n_mh if n_adapt is None else n_adapt
    full = math.isinf(gamma)
    gamma_l = 0.0 if full else f32(gamma * n_leapfrog)
    temp32, sqrt_temp, beta = f32(temp), f32(math.sqrt(temp)), f32(1.0 / temp)
    delta32 = f32(delta)
    mu32 = f32(math.log(mu_factor * eps0) if mu is None else mu)
    log_min, log_max = f32(math.log(bounds[0])), f32(math.log(bounds[1]))
    tab = table(n_adapt, m0).tolist()
    x = x0.to(dtype).clone()
    v = (sqrt_temp * xi0.to(dtype)) if v0 is None else v0.to(dtype).clone()
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
            c1, c2 = 0.0, sqrt_temp
        else:
            span = gamma_l * eps
            c1 = torch.exp(-span)[:, None]
            c2 = torch.sqrt(temp32 * (-torch.expm1(-2.0 * span)))[:, None]
        v = c1 * v + c2 * z[t].to(dtype)  # O: two products and a sum
        h0 = _hamiltonian(energy.energy(x), v)
        xp, w = x, v
        for _ in range(n_leapfrog):  # oracle/hmc.py leapfrog(), safe mode, identity mass, the chain's own step size
            w_half = w + 0.5 * e * _force(energy, xp)
            xp = xp + e * w_half
            w = w_half + 0.5 * e * _force(energy, xp)
            xp = xp.nan_to_num_(nan=0.0)
            w = w.nan_to_num_(nan=0.0)
        h1 = _hamiltonian(energy.energy(xp), w)
        a = torch.exp((beta * (h0 - h1)).clamp_(min=-50.0, max=50.0)).clamp_(max=1.0)
        ut = u[t].to(dtype)
        acc = ut < a
        accepted.append(acc)
        margins.append(torch.where(a == a, (ut - a).abs().double(), torch.full((), float("inf"), dtype=torch.float64)))
        x = torch.where(acc[:, None], xp, x)
        v = torch.where(acc[:, None], w, -v)  # the flip
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
    return {"x": x, "v": v, "traj": torch.stack(kept, dim=1) if kept else torch.zeros(n, 0, dim, dtype=dtype),
            "accepted": torch.stack(accepted), "margin": min((m.min().item() for m in margins), default=float("inf")),
            "da": torch.stack((eps, hbar, lbar)), "eps_trace": torch.stack(trace), "alphas": torch.stack(alphas),
            "alpha_mean": alpha_sum / n_adapt if n_adapt > 0 else alpha_sum}


# ghmc_cases' grid with n_mh in {2, 4, 6} in place of {1, 4, 6}: the controller acts in every case
CASES = {kind: [(k, dim, n, 2 if n_mh == 1 else n_mh, thin, L) for k, dim, n, n_mh, thin, L in group]
         for kind, group in GHMC_CASES.items()}
ALL_CASES = [c for group in CASES.values() for c in group]


@functools.lru_cache(maxsize=None)
def case(kind, dim, n, n_mh, thin, L, gamma=GAMMA, temp=TEMP):
    """Inputs and both restatements of a case, computed once per session and shared (read-only): ghmc_cases.case's rule -- the
    seed is the first whose fp64 restatement has no decision closer than MARGIN_BAR to its threshold and whose fp32 restatement
    decides alike.  `found` says whether one of the 200 did."""
    from helpers import to64

    spec = energy_spec(kind, dim)
    eps0 = step_size(kind, dim)
    found = False
    for seed in range(200):
        x0, v0, z, u = draw_inputs(7100 + seed, kind, n, dim, n_mh)
        ref64 = restate(to64(oracle_of(spec)), x0, v0, z, u, eps0, L, gamma, temp, torch.float64, thin)
        if ref64["margin"] <= MARGIN_BAR:
            continue
        ref32 = restate(oracle_of(spec), x0, v0, z, u, eps0, L, gamma, temp, torch.float32, thin)
        if torch.equal(ref32["accepted"], ref64["accepted"]):
            found = True
            break
    return {"spec": spec, "x0": x0, "v0": v0, "z": z, "u": u, "eps0": eps0, "L": L, "gamma": gamma, "temp": temp, "ref32": ref32,
            "ref64": ref64, "seed": seed, "found": found, "shape": (n, dim), "n_mh": n_mh, "thin": thin,
            "mu": math.log(MU_FACTOR * eps0)}


# ---- the law: the pooled step size of two independent implementations agrees within their standard errors
LAW_SIGMAS = 4.5
LAW = dict(kind="harmonic", dim=4, n=4096, n_mh=200, L=4, delta=0.8, eps0=0.05)


def pooled_log(step_sizes):
    """log of the pooled step size (the median of the finite logs) and its standard error 1.2533 std / sqrt(n)."""
    logs = step_sizes.double().log()
    logs = logs[torch.isfinite(logs)]
    return logs.median().item(), 1.2533 * logs.std().item() / math.sqrt(logs.numel())
