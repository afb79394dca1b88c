"""BAOAB and generalized HMC with a scalar or diagonal mass on the MLP energy (include/ebm_hip_mass_mlp.h,
ebm_kinetic_mlp_chain_mass_f32 and ebm_ghmc_mlp_chain_mass_f32): the cases the tests run and their inputs.  Nothing is restated here: mass_cases.restate_baoab
and mass_cases.restate_ghmc take any object with energy() / grad(), and kinetic_mlp_cases.CpuMlpEnergy is one.  Shared by
test_mass_mlp.py (CPU tier) and test_mass_mlp_gpu.py; it never calls the package's samplers."""

import copy
import functools
import math

import torch

import ghmc_mlp_cases
import kinetic_mlp_cases
import mass_cases
from ghmc_mlp_cases import MAX_SEEDS, MIN_DECISIONS  # noqa: F401  (re-exported for the tests)
from kinetic_mlp_cases import CpuMlpEnergy
from mass_cases import MARGIN_BAR, mass_of, start_momentum  # noqa: F401

GAMMA, TEMP = 1.5, 0.8
BAOAB_STEP, GHMC_STEP = 0.2, 1.0  # times sqrt(min m): h^2 E'' / m is at most what the unit-mass MLP cases run at

# (in_dim, hidden, n, k_steps, thin, mass form): every (HT, DT), both Philox paths (dim % 4 != 0: 1, 2, 5, 30, 33, 65), partial
# waves (37), several workgroups and a tail (257, 129), padded columns (1, 2, 5, 30, 33, 40, 65, 100) where a padding slot's mass
# can go wrong
BAOAB_CASES = [
    (2, 64, 257, 11, 3, "diag"),
    (1, 64, 37, 4, 2, "scalar"),
    (5, 128, 37, 4, 2, "diag"),
    (30, 128, 257, 1, 1, "scalar"),
    (33, 128, 37, 4, 2, "diag"),
    (40, 64, 37, 4, 2, "scalar"),
    (64, 128, 129, 4, 2, "diag"),
    (65, 64, 37, 1, 1, "diag"),
    (96, 128, 37, 4, 2, "scalar"),
    (100, 64, 129, 4, 2, "diag"),
    (128, 64, 37, 4, 2, "scalar"),
    (128, 128, 37, 11, 3, "diag"),
]
# (in_dim, hidden, n, n_mh, thin, L, mass form): the same twelve shapes
GHMC_CASES = [
    (2, 64, 257, 6, 3, 1, "diag"),
    (1, 64, 37, 4, 2, 3, "scalar"),
    (5, 128, 37, 4, 2, 1, "diag"),
    (30, 128, 257, 1, 1, 3, "scalar"),
    (33, 128, 37, 4, 2, 3, "diag"),
    (40, 64, 37, 4, 2, 1, "scalar"),
    (64, 128, 129, 4, 2, 1, "diag"),
    (65, 64, 37, 1, 1, 3, "diag"),
    (96, 128, 37, 4, 2, 1, "scalar"),
    (100, 64, 129, 4, 2, 3, "diag"),
    (128, 64, 37, 4, 2, 1, "scalar"),
    (128, 128, 37, 6, 3, 3, "diag"),
]
# one shape per (HT, DT) for the bit-for-bit anchors: (in_dim, hidden)
ANCHOR_SHAPES = [(5, 64), (40, 64), (65, 64), (128, 64), (30, 128), (64, 128), (96, 128), (128, 128)]
PHILOX_DIMS = [(5, 128), (33, 128), (40, 64), (128, 64)]  # native draws against the materialised fields


def baoab_step(mass):
    return BAOAB_STEP * math.sqrt(mass_cases.min_mass(mass))


def ghmc_step(mass):
    return GHMC_STEP * math.sqrt(mass_cases.min_mass(mass))


@functools.lru_cache(maxsize=None)
def baoab_case(in_dim, hidden, n, k, thin, form):
    """Inputs and both restatements of a case, computed once per session and shared (read-only)."""
    cpu, mass = kinetic_mlp_cases.net(in_dim, hidden), mass_of(form, in_dim)
    g = torch.Generator().manual_seed(7000 + in_dim + n)
    x0 = torch.randn(n, in_dim, generator=g)
    p0 = start_momentum(mass, torch.randn(n, in_dim, generator=g))
    noise = torch.randn(k, n, in_dim, generator=g)
    h = baoab_step(mass)
    ref32 = mass_cases.restate_baoab(CpuMlpEnergy(cpu), x0, p0, noise, h, GAMMA, TEMP, mass, thin, torch.float32)
    ref64 = mass_cases.restate_baoab(CpuMlpEnergy(copy.deepcopy(cpu).double()), x0, p0, noise, h, GAMMA, TEMP, mass, thin, torch.float64)
    return {"cpu": cpu, "mass": mass, "x0": x0, "v0": p0, "noise": noise, "h": h, "ref32": ref32, "ref64": ref64,
            "shape": (n, in_dim), "k": k, "thin": thin}


def ghmc_inputs(seed, in_dim, n, n_mh, mass):
    g = torch.Generator().manual_seed(7500 + seed + in_dim + n)
    x0 = torch.randn(n, in_dim, generator=g)
    p0 = start_momentum(mass, torch.randn(n, in_dim, generator=g))
    return x0, p0, torch.randn(n_mh, n, in_dim, generator=g), torch.rand(n_mh, n, generator=g)


@functools.lru_cache(maxsize=None)
def ghmc_case(in_dim, hidden, n, n_mh, thin, L, form):
    """Inputs and both restatements of a case (the seed rule of ghmc_mlp_cases.case): the first of MAX_SEEDS seeds whose fp64
    restatement decides nothing within MARGIN_BAR of its threshold and whose fp32 restatement decides alike; "found" says whether
    one did."""
    cpu, mass = ghmc_mlp_cases.net(in_dim, hidden), mass_of(form, in_dim)
    e32, e64 = CpuMlpEnergy(cpu), CpuMlpEnergy(copy.deepcopy(cpu).double())
    eps = ghmc_step(mass)
    found, ref32 = False, None
    for seed in range(MAX_SEEDS):
        x0, p0, z, u = ghmc_inputs(seed, in_dim, n, n_mh, mass)
        ref64 = mass_cases.restate_ghmc(e64, x0, p0, z, u, eps, L, GAMMA, TEMP, mass, torch.float64, thin)
        ref32 = None
        if ref64["margin"] <= MARGIN_BAR:
            continue
        ref32 = mass_cases.restate_ghmc(e32, x0, p0, z, u, eps, L, GAMMA, TEMP, mass, torch.float32, thin)
        if torch.equal(ref32["accepted"], ref64["accepted"]):
            found = True
            break
    if ref32 is None:
        ref32 = mass_cases.restate_ghmc(e32, x0, p0, z, u, eps, L, GAMMA, TEMP, mass, torch.float32, thin)
    return {"cpu": cpu, "mass": mass, "x0": x0, "v0": p0, "z": z, "u": u, "eps": eps, "L": L, "gamma": GAMMA, "temp": TEMP,
            "ref32": ref32, "ref64": ref64, "seed": seed, "found": found, "shape": (n, in_dim), "n_mh": n_mh, "thin": thin}


def restatement_errors(c):
    """{key: (fp32 restatement's max error against fp64, max |fp64|)} for x, v and traj of a case."""
    out = {}
    for key in ("x", "v", "traj"):
        ref = c["ref64"][key]
        out[key] = ((c["ref32"][key].double() - ref).abs().max().item(), ref.abs().max().item())
    return out


def anchor_inputs(in_dim, n=37, k=4):
    """A start state, a momentum plane, step noise [k, n, dim] and uniforms [k, n] for the bit-for-bit runs."""
    g = torch.Generator().manual_seed(7900 + in_dim)
    return (torch.randn(n, in_dim, generator=g), math.sqrt(TEMP) * torch.randn(n, in_dim, generator=g),
            torch.randn(k, n, in_dim, generator=g), torch.rand(k, n, generator=g))
