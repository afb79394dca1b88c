"""Generalized HMC: an independent restatement of the algorithm (include/ebm_hip.h, ebm_ghmc_chain_f32) in torch ops on the
oracle energies -- the O step and the flip spelled operation for operation, the trajectory the literal safe-mode leapfrog
sequence tempering_hmc_cases.restate uses -- the cases the tests run, and their inputs.  Shared by test_ghmc.py (CPU tier) and
test_ghmc_gpu.py; it never calls the package's sampler."""

import functools
import math

import torch

from tempering_cases import energy_spec, model_of, oracle_of, start_scale  # noqa: F401  (re-exported for the tests)
from tempering_hmc_cases import MARGIN_BAR, leapfrog_steps, step_c  # noqa: F401


def constants(eps, n_leapfrog, gamma, temp):
    """c1, c2, sqrt_temp, beta: formed in double, each rounded once to fp32 (returned as the Python floats of those fp32
    values); gamma = inf gives c1 = 0 and c2 = sqrt_temp exactly."""
    sqrt_temp = math.sqrt(temp)
    if math.isinf(gamma):
        c1, c2 = 0.0, sqrt_temp
    else:
        span = gamma * eps * n_leapfrog
        c1, c2 = math.exp(-span), math.sqrt(temp * (-math.expm1(-2.0 * span)))
    return [torch.tensor(v, dtype=torch.float64).to(torch.float32).item() for v in (c1, c2, sqrt_temp, 1.0 / temp)]


def _force(energy, x):
    return (-energy.grad(x)).clamp_(min=-1e6, max=1e6)


def _hamiltonian(e, v):
    return e.clamp(min=-1e10, max=1e10) + (0.5 * torch.sum(v.square(), dim=-1)).clamp_(min=0.0, max=1e10)


def restate(energy, x0, v0, z, u, eps, n_leapfrog, gamma, temp, dtype=torch.float32, thin=1, xi0=None):
    """x0 [n, dim], v0 [n, dim] (or None: sqrt_temp * xi0), z [n_mh, n, dim], u [n_mh, n] -> the final x and v, the kept
    positions [n, n_mh // thin, dim], the decisions [n_mh, n] and the closest call min |u - a| (inf when the threshold is NaN).
    Every operation rounded on its own in `dtype`; float64 runs the same fp32 constants, upcast."""
    c1, c2, sqrt_temp, beta = constants(eps, n_leapfrog, gamma, temp)
    eps_t = torch.tensor(float(eps), dtype=dtype)  # (oracle/hmc.py: eps as a tensor of the state's dtype)
    x = x0.to(dtype).clone()
    v = (sqrt_temp * xi0.to(dtype)) if v0 is None else v0.to(dtype).clone()
    accepted, margins, kept = [], [], []
    for t in range(z.shape[0]):
        v = c1 * v + c2 * z[t].to(dtype)  # O: two products and a sum
        h0 = _hamiltonian(energy.energy(x), v)
        xp, w = x, v
        for _ in range(n_leapfrog):  # oracle/hmc.py leapfrog(), safe mode, identity mass
            w_half = w + 0.5 * eps_t * _force(energy, xp)
            xp = xp + eps_t * w_half
            w = w_half + 0.5 * eps_t * _force(energy, xp)
            xp = xp.nan_to_num_(nan=0.0)
            w = w.nan_to_num_(nan=0.0)
        h1 = _hamiltonian(energy.energy(xp), w)
        a = torch.exp((beta * (h0 - h1)).clamp_(min=-50.0, max=50.0)).clamp_(max=1.0)
        ut = u[t].to(dtype)
        acc = ut < a
        accepted.append(acc)
        margins.append(torch.where(a == a, (ut - a).abs().double(), torch.full((), float("inf"), dtype=torch.float64)))
        x = torch.where(acc[:, None], xp, x)
        v = torch.where(acc[:, None], w, -v)  # the flip: the negative of the velocity after O
        if (t + 1) % thin == 0:
            kept.append(x.clone())
    n, dim = x0.shape
    return {"x": x, "v": v, "traj": torch.stack(kept, dim=1) if kept else torch.zeros(n, 0, dim, dtype=dtype),
            "accepted": torch.stack(accepted) if accepted else torch.zeros(0, n, dtype=torch.bool),
            "margin": min((m.min().item() for m in margins), default=float("inf"))}


# Friction and temperature of every case (neither is 1: c1, c2, sqrt_temp and beta are all exercised).
GAMMA, TEMP = 1.5, 0.8


def step_size(kind, dim):
    """tempering_hmc_cases' step size of slot 0: c (2 / dim)^(1/4)."""
    return step_c(kind, dim) * (2.0 / dim) ** 0.25


# (kind, dim, n, n_mh, thin, L): the thinning of the full grid that kinetic_cases.py uses.  dims: the smallest of every lane
# geometry -- 2 one lane per chain, 5 G = 2 masked, 12 G = 4 masked, 32 G = 8 full, 64 G = 16 full, 100 G = 32 masked, 256
# G = 64 full.  n: 9 a partial wave, 37 an odd count, 257 several workgroups and a tail.  (n_mh, thin): (1, 1) one transition,
# (4, 2), (6, 3).  L: 1 (a trajectory that starts and ends with its half kicks) and 3 (merged kicks between).
def _grid(kind, shapes):
    return [(kind, dim, n, n_mh, thin, (1, 3)[i % 2]) for i, (dim, n, n_mh, thin) in enumerate(shapes)]


_SHAPES_A = [(2, 257, 4, 2), (5, 37, 6, 3), (12, 9, 1, 1), (32, 37, 4, 2), (64, 257, 6, 3), (100, 9, 6, 3), (256, 37, 1, 1)]
_SHAPES_B = [(2, 9, 6, 3), (5, 257, 1, 1), (12, 37, 4, 2), (32, 257, 6, 3), (64, 9, 4, 2), (100, 37, 1, 1), (256, 257, 4, 2)]
_LANDSCAPE_SHAPES = [(2, 257, 4, 2), (5, 37, 6, 3), (12, 37, 4, 2), (32, 37, 6, 3), (64, 37, 4, 2), (100, 37, 1, 1), (256, 9, 6, 3)]
CASES = {
    "double_well": _grid("double_well", _SHAPES_A),
    "harmonic": _grid("harmonic", _SHAPES_B),
    "gaussian": _grid("gaussian", [(5, 37, 6, 3), (32, 257, 4, 2), (100, 37, 1, 1), (256, 9, 4, 2)]),
    "gmm": _grid("gmm", [(2, 257, 4, 2), (32, 37, 6, 3), (100, 37, 4, 2)]),
    "rastrigin": _grid("rastrigin", [(5, 37, 6, 3), (32, 257, 4, 2)]),
    "rosenbrock": _grid("rosenbrock", _LANDSCAPE_SHAPES),
    "ackley": _grid("ackley", _LANDSCAPE_SHAPES),
}
ALL_CASES = [c for group in CASES.values() for c in group]


def draw_inputs(seed, kind, n, dim, n_mh):
    g = torch.Generator().manual_seed(seed)
    x0 = start_scale(kind) * torch.randn(n, dim, generator=g)
    v0 = math.sqrt(TEMP) * torch.randn(n, dim, generator=g)
    return x0, v0, torch.randn(n_mh, n, dim, generator=g), torch.rand(n_mh, n, generator=g)


@functools.lru_cache(maxsize=None)
def case(kind, dim, n, n_mh, thin, L, eps=None, gamma=GAMMA, temp=TEMP):
    """Inputs and both restatements of a case, computed once per session and shared (read-only).  The seed is the first whose
    fp64 restatement has no decision closer than MARGIN_BAR to its threshold and whose fp32 restatement decides alike."""
    from helpers import to64

    spec = energy_spec(kind, dim)
    eps = step_size(kind, dim) if eps is None else eps
    for seed in range(200):
        x0, v0, z, u = draw_inputs(7100 + seed, kind, n, dim, n_mh)
        ref64 = restate(to64(oracle_of(spec)), x0, v0, z, u, eps, L, gamma, temp, torch.float64, thin)
        if ref64["margin"] <= MARGIN_BAR:
            continue
        ref32 = restate(oracle_of(spec), x0, v0, z, u, eps, L, gamma, temp, torch.float32, thin)
        if torch.equal(ref32["accepted"], ref64["accepted"]):
            break
    return {"spec": spec, "x0": x0, "v0": v0, "z": z, "u": u, "eps": eps, "L": L, "gamma": gamma, "temp": temp, "ref32": ref32,
            "ref64": ref64, "seed": seed, "shape": (n, dim), "n_mh": n_mh, "thin": thin}


# ---- the law on a quadratic: exact for every step size, var(x) k / T = 1 and var(v) / T = 1
LAW_SIGMAS = 4.5  # the factor test_moments.py and kinetic_cases.py use
# (k, eps, gamma, T, L) and the transitions run
LAWS = [(4.0, 0.3, 1.0, 1.0, 1), (1.0, 1.0, 0.5, 2.0, 1), (4.0, 0.3, 1.0, 1.0, 4)]
LAW_SHAPE, LAW_STEPS, LAW_SEED = (4096, 4), 400, 0


def law_bar(n_values):
    """4.5 standard errors of the variance of n_values independent normal values, relative."""
    return LAW_SIGMAS * math.sqrt(2.0 / (n_values - 1))
