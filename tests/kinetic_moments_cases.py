"""Running moments of the BAOAB and generalized-HMC walkers (include/ebm_hip.h, ebm_kinetic_moments_f32): the recurrences of the
accumulators restated in torch ops, the transitions taken from kinetic_cases.py and ghmc_cases.py (independent restatements that
never call the package's samplers), the cases the tests run, and their inputs.  Shared by test_kinetic_moments.py (CPU tier)
and test_kinetic_moments_gpu.py."""

import functools

import torch

import ghmc_cases
import kinetic_cases
from moments_cases import recip_table, split, two_pass, welford  # noqa: F401  (re-exported for the tests)
from tempering_cases import energy_spec, model_of, oracle_of, start_scale  # noqa: F401
from tempering_hmc_cases import MARGIN_BAR  # noqa: F401

GAMMA, TEMP = kinetic_cases.GAMMA, kinetic_cases.TEMP
assert (GAMMA, TEMP) == (ghmc_cases.GAMMA, ghmc_cases.TEMP)
ELEMENTWISE = ("double_well", "harmonic")


def v2_mean(v_traj, h, dtype=torch.float32):
    """v_traj [n, 2 h, ...] -> the running mean of v^2 of either half, [2, n, ...]: m = m + (v v - m) recip[c - 1], every
    operation rounded on its own in `dtype`, with the fp32 reciprocal table."""
    assert v_traj.shape[1] == 2 * h
    rc = recip_table(h).to(dtype)
    t = v_traj.to(dtype)
    m = torch.zeros((2, t.shape[0]) + tuple(t.shape[2:]), dtype=dtype)
    for j in range(2 * h):
        half, c = divmod(j, h)
        v = t[:, j]
        m[half] = m[half] + (v * v - m[half]) * rc[c]
    return m


def restate_baoab(energy, x0, v0, noise, h, gamma, temp, burn_in, dtype=torch.float32, xi0=None):
    """kinetic_cases.restate, one step per call (the kicks are not merged and the gradient is a function of the position: the
    bits do not depend on where a run is cut) -> the final x and v, the counted positions [n, 2 h, dim], the velocities at the
    end of those steps and the energies of those positions [n, 2 h]."""
    k = noise.shape[0]
    split(k, burn_in)
    x, v = x0, v0
    kept, v_kept, e_kept = [], [], []
    for s in range(k):
        r = kinetic_cases.restate(energy, x, v, noise[s:s + 1], h, gamma, temp, 1, dtype, xi0=xi0 if s == 0 else None)
        x, v = r["x"], r["v"]
        if s >= burn_in:
            kept.append(x.clone())
            v_kept.append(v.clone())
            e_kept.append(energy.energy(x))
    return {"x": x, "v": v, "traj": torch.stack(kept, dim=1), "v_traj": torch.stack(v_kept, dim=1), "e_traj": torch.stack(e_kept, dim=1)}


def restate_ghmc(energy, x0, v0, z, u, eps, n_leapfrog, gamma, temp, burn_in, dtype=torch.float32, xi0=None):
    """ghmc_cases.restate with every transition kept -> the final x and v, the decisions, the closest call, the counted (held)
    positions [n, 2 h, dim] and their energies [n, 2 h]."""
    split(z.shape[0], burn_in)
    r = ghmc_cases.restate(energy, x0, v0, z, u, eps, n_leapfrog, gamma, temp, dtype, 1, xi0=xi0)
    traj = r["traj"][:, burn_in:]
    n, m, dim = traj.shape
    r["traj"] = traj
    r["e_traj"] = energy.energy(traj.reshape(n * m, dim)).view(n, m)
    return r


# (kind, dim, n, k_steps, burn_in): every lane geometry -- dim 2 one lane per chain, 5 G = 2 masked, 12 G = 4 masked, 32 G = 8
# full, 100 G = 32 masked, 256 G = 64 full; 9 chains a partial wave, 37 an odd count, 257 several workgroups and a tail; (4, 0)
# the shortest halves (h = 2), (11, 3) and (40, 6) a burn-in in front of h = 4 and h = 17.  Every one of the seven kinds under
# both samplers; generalized HMC alternates L = 1 and L = 3 down the list.
CASES = [
    ("double_well", 2, 257, 4, 0),
    ("double_well", 5, 37, 11, 3),
    ("double_well", 32, 37, 40, 6),
    ("double_well", 100, 9, 11, 3),
    ("double_well", 256, 37, 4, 0),
    ("harmonic", 12, 257, 11, 3),
    ("harmonic", 100, 37, 40, 6),
    ("gaussian", 5, 37, 11, 3),
    ("gaussian", 256, 9, 4, 0),
    ("gmm", 32, 37, 40, 6),
    ("gmm", 2, 257, 4, 0),
    ("rosenbrock", 12, 37, 11, 3),
    ("rosenbrock", 256, 9, 40, 6),
    ("ackley", 100, 37, 11, 3),
    ("ackley", 5, 9, 40, 6),
    ("rastrigin", 32, 257, 4, 0),
    ("rastrigin", 5, 37, 11, 3),
]
GHMC_CASES = [c + ((1, 3)[i % 2],) for i, c in enumerate(CASES)]


@functools.lru_cache(maxsize=None)
def baoab_case(kind, dim, n, k, burn_in):
    """kinetic_cases.case with every step kept: inputs and both restatements, computed once per session and shared (read-only)."""
    c = kinetic_cases.case(kind, dim, n, k, 1)
    return {**c, "burn_in": burn_in, "half": split(k, burn_in)}


@functools.lru_cache(maxsize=None)
def ghmc_case(kind, dim, n, k, burn_in, L):
    """ghmc_cases.case with every transition kept: the seed is the first whose fp64 restatement has no decision closer than
    MARGIN_BAR to its threshold and whose fp32 restatement decides alike."""
    c = ghmc_cases.case(kind, dim, n, k, 1, L)
    return {**c, "burn_in": burn_in, "half": split(k, burn_in)}
