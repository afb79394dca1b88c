"""Underdamped Langevin, BAOAB: an independent restatement of the algorithm (include/ebm_hip.h, ebm_kinetic_chain_f32) in torch
ops on the oracle energies, the cases the tests run, and their inputs.  Shared by test_kinetic.py (CPU tier) and
test_kinetic_gpu.py; it never calls the package's sampler."""

import functools
import math

import torch

from tempering_cases import energy_spec, model_of, oracle_of, start_scale  # noqa: F401


def constants(h, gamma, temp):
    """hh, c1, c2, sqrt_temp: formed in double, each rounded once to fp32 (returned as the Python floats of those fp32 values)."""
    vals = [h / 2.0, math.exp(-gamma * h), math.sqrt(temp * (-math.expm1(-2.0 * gamma * h))), math.sqrt(temp)]
    return [torch.tensor(v, dtype=torch.float64).to(torch.float32).item() for v in vals]


def restate(energy, x0, v0, noise, h, gamma, temp, thin=1, dtype=torch.float32, xi0=None):
    """x0 [n, dim], v0 [n, dim] (or None: sqrt_temp * xi0), noise [k, n, dim] -> the final x and v and the kept positions
    [n, k // thin, dim].  Every operation rounded on its own in `dtype`; float64 runs the same fp32 constants, upcast."""
    hh, c1, c2, sqrt_temp = constants(h, gamma, temp)
    x = x0.to(dtype).clone()
    v = (sqrt_temp * xi0.to(dtype)) if v0 is None else v0.to(dtype).clone()
    g = energy.grad(x)
    kept = []
    for s in range(noise.shape[0]):
        v = v - hh * g
        x = x + hh * v
        v = c1 * v + c2 * noise[s].to(dtype)
        x = x + hh * v
        g = energy.grad(x)
        v = v - hh * g
        if (s + 1) % thin == 0:
            kept.append(x.clone())
    n, dim = x0.shape
    return {"x": x, "v": v, "traj": torch.stack(kept, dim=1) if kept else torch.zeros(n, 0, dim, dtype=dtype)}


# Friction and temperature of every case (neither is 1: c1, c2 and sqrt_temp are all exercised), and the step size per kind:
# inside the stability limit h^2 E'' < 4 from the normal starts of the cases -- the double well (barrier 2) has E'' = 2 (12 x^2 - 4)
# up to a few hundred at |x| = 4; Rosenbrock (b = 4) and the rippled landscapes likewise; the Gaussians (precision eigenvalues
# at most 1 / 0.5 = 2) and the harmonic well (k = 1.5) have h^2 lambda_max <= 0.18 < 1.
GAMMA, TEMP = 1.5, 0.8
STEP = {"double_well": 0.05, "harmonic": 0.3, "gaussian": 0.3, "gmm": 0.3, "rosenbrock": 0.03, "ackley": 0.05, "rastrigin": 0.05}
ELEMENTWISE = ("double_well", "harmonic")

# (kind, dim, n, k_steps, thin).  dims: the smallest of every lane geometry -- 2 one lane per chain, 5 G = 2 masked, 12 G = 4
# masked, 32 G = 8 full, 64 G = 16 full, 100 G = 32 masked, 256 G = 64 full.  n: 9 a partial wave, 37 an odd count, 257 several
# workgroups and a tail.  (k, thin): (1, 1) one step, (4, 2), (11, 3) with two steps behind the last kept one.
EXACT_CASES = [
    ("double_well", 2, 257, 4, 2),
    ("double_well", 5, 37, 11, 3),
    ("double_well", 12, 9, 1, 1),
    ("double_well", 32, 37, 4, 2),
    ("double_well", 64, 257, 11, 3),
    ("double_well", 100, 9, 11, 3),
    ("double_well", 256, 37, 1, 1),
    ("harmonic", 2, 9, 11, 3),
    ("harmonic", 5, 257, 1, 1),
    ("harmonic", 12, 37, 4, 2),
    ("harmonic", 32, 257, 11, 3),
    ("harmonic", 64, 9, 4, 2),
    ("harmonic", 100, 37, 1, 1),
    ("harmonic", 256, 257, 4, 2),
]
# the coupled kinds at the dims their fused tests use (tempering_cases.py, moments_cases.py)
_LANDSCAPE_SHAPES = [(2, 257, 4, 2), (5, 37, 11, 3), (12, 37, 4, 2), (32, 37, 11, 3), (64, 37, 4, 2), (100, 37, 1, 1), (256, 9, 11, 3)]
COUPLED_CASES = ([
    ("gaussian", 5, 37, 11, 3),
    ("gaussian", 32, 257, 4, 2),
    ("gaussian", 100, 37, 1, 1),
    ("gaussian", 256, 9, 4, 2),
    ("gmm", 2, 257, 4, 2),
    ("gmm", 32, 37, 11, 3),
    ("gmm", 100, 37, 4, 2),
    ("rastrigin", 5, 37, 11, 3),
    ("rastrigin", 32, 257, 4, 2),
] + [("rosenbrock",) + s for s in _LANDSCAPE_SHAPES] + [("ackley",) + s for s in _LANDSCAPE_SHAPES])


@functools.lru_cache(maxsize=None)
def case(kind, dim, n, k, thin):
    """Inputs and both restatements of a case, computed once per session and shared (read-only)."""
    from helpers import to64

    spec = energy_spec(kind, dim)
    g = torch.Generator().manual_seed(7000 + dim + n)
    x0 = start_scale(kind) * torch.randn(n, dim, generator=g)
    v0 = math.sqrt(TEMP) * torch.randn(n, dim, generator=g)
    noise = torch.randn(k, n, dim, generator=g)
    h = STEP[kind]
    ref32 = restate(oracle_of(spec), x0, v0, noise, h, GAMMA, TEMP, thin, torch.float32)
    ref64 = restate(to64(oracle_of(spec)), x0, v0, noise, h, GAMMA, TEMP, thin, torch.float64)
    return {"spec": spec, "x0": x0, "v0": v0, "noise": noise, "h": h, "ref32": ref32, "ref64": ref64, "shape": (n, dim), "k": k,
            "thin": thin}


# ---- the law on a quadratic: BAOAB's position marginal is exact, var(x) k / T = 1, and var(v) / T = 1 - h^2 k / 4
LAW_SIGMAS = 4.5  # the factor test_moments.py uses


def law_bar(n_values):
    """4.5 standard errors of the variance of n_values independent normal values, relative."""
    return LAW_SIGMAS * math.sqrt(2.0 / (n_values - 1))
