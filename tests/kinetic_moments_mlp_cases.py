"""Running moments of the BAOAB and generalized-HMC walks on the MLP energy (include/ebm_hip.h, ebm_kinetic_moments_mlp_f32): the
cases the tests run and their restatements, composed from what exists -- the networks and the autograd oracle of
kinetic_mlp_cases.py, the sharpened networks, inputs and seed search of ghmc_mlp_cases.py (thin = 1 keeps every transition), the
one-step-per-call BAOAB restatement and the v^2 recurrence of kinetic_moments_cases.py, the Welford recurrence and the reciprocal
table of moments_cases.py.  Shared by test_kinetic_moments_mlp.py (CPU tier) and test_kinetic_moments_mlp_gpu.py; it never calls the
package's samplers."""

import copy
import functools
import math

import torch

import ghmc_mlp_cases
import kinetic_mlp_cases
from ghmc_mlp_cases import MARGIN_BAR, MAX_SEEDS, MIN_DECISIONS  # noqa: F401  (re-exported for the tests)
from kinetic_mlp_cases import CpuMlpEnergy
from kinetic_moments_cases import restate_baoab, v2_mean  # noqa: F401
from moments_cases import recip_table, split, welford  # noqa: F401

GAMMA, TEMP, STEP = kinetic_mlp_cases.GAMMA, kinetic_mlp_cases.TEMP, kinetic_mlp_cases.STEP
assert (GAMMA, TEMP) == (ghmc_mlp_cases.GAMMA, ghmc_mlp_cases.TEMP)
EPS = ghmc_mlp_cases.EPS

# (in_dim, hidden, n, k, burn_in, L): every (HT, DT) -- hidden 64 / 128 at dims 1 .. 32, 33 .. 64, 65 .. 96, 97 .. 128 --, the
# per-element Philox path (dim % 4 != 0) and the per-quad one, a partial wave (37 = 32 + 5 chains), several workgroups and a tail
# (257 = 2 x 128 + 1), the shortest halves h = 2, h = 3, and a burn-in in front of the halves.
GHMC_CASES = [
    (2, 64, 257, 6, 0, 1),
    (1, 64, 37, 4, 0, 3),
    (5, 128, 37, 4, 0, 1),
    (30, 128, 257, 7, 3, 3),
    (32, 64, 129, 6, 2, 1),
    (33, 128, 37, 4, 0, 3),
    (40, 64, 37, 4, 0, 1),
    (64, 128, 129, 4, 0, 1),
    (65, 64, 37, 5, 1, 3),
    (96, 128, 37, 4, 0, 1),
    (100, 64, 129, 4, 0, 3),
    (128, 64, 37, 4, 0, 1),
    (128, 128, 37, 6, 2, 3),
]
# the same (in_dim, hidden, n); (k, burn_in) = (4, 0), (7, 3), (11, 3) down the list
_BAOAB_RUNS = [(4, 0), (7, 3), (11, 3)]
BAOAB_CASES = [(c[0], c[1], c[2], *_BAOAB_RUNS[i % 3]) for i, c in enumerate(GHMC_CASES)]


def _energies(oracle, traj):
    n, m, dim = traj.shape
    return oracle.energy(traj.reshape(n * m, dim)).view(n, m)


@functools.lru_cache(maxsize=None)
def ghmc_case(in_dim, hidden, n, k, burn_in, L, gamma=GAMMA):
    """ghmc_mlp_cases.case with every transition kept, cut to the counted ones: inputs, both restatements (x, v, accepted, the
    counted positions traj [n, 2 h, dim] and their energies e_traj [n, 2 h] from the restatement's own network), the seed and
    whether the search found it.  Computed once per session and shared (read-only)."""
    c = ghmc_mlp_cases.case(in_dim, hidden, n, k, 1, L, gamma)
    h = split(k, burn_in)
    e32, e64 = CpuMlpEnergy(c["cpu"]), CpuMlpEnergy(copy.deepcopy(c["cpu"]).double())
    out = {**c, "k": k, "burn_in": burn_in, "half": h}
    for key, oracle in (("ref32", e32), ("ref64", e64)):
        r = dict(c[key])
        r["traj"] = c[key]["traj"][:, burn_in:].contiguous()
        r["e_traj"] = _energies(oracle, r["traj"])
        out[key] = r
    return out


@functools.lru_cache(maxsize=None)
def baoab_case(in_dim, hidden, n, k, burn_in):
    """Inputs and both restatements (kinetic_moments_cases.restate_baoab on the network of kinetic_mlp_cases.net) of a BAOAB case:
    x, v, traj, v_traj [n, 2 h, dim], e_traj [n, 2 h].  Computed once per session and shared (read-only)."""
    cpu = kinetic_mlp_cases.net(in_dim, hidden)
    g = torch.Generator().manual_seed(7000 + in_dim + n)
    x0 = torch.randn(n, in_dim, generator=g)
    v0 = math.sqrt(TEMP) * torch.randn(n, in_dim, generator=g)
    noise = torch.randn(k, n, in_dim, generator=g)
    ref32 = restate_baoab(CpuMlpEnergy(cpu), x0, v0, noise, STEP, GAMMA, TEMP, burn_in, torch.float32)
    ref64 = restate_baoab(CpuMlpEnergy(copy.deepcopy(cpu).double()), x0, v0, noise, STEP, GAMMA, TEMP, burn_in, torch.float64)
    return {"cpu": cpu, "x0": x0, "v0": v0, "noise": noise, "h": STEP, "ref32": ref32, "ref64": ref64, "shape": (n, in_dim), "k": k,
            "burn_in": burn_in, "half": split(k, burn_in)}


def restatement_errors(c, keys):
    """{key: (fp32 restatement's max error against fp64, max |fp64|)} of a case."""
    out = {}
    for key in keys:
        ref = c["ref64"][key]
        out[key] = ((c["ref32"][key].double() - ref).abs().max().item(), ref.abs().max().item())
    return out


def moments_of(traj, e_traj, v_traj, h):
    """The entry's mom [4, n, dim], e_mom [4, n] and v2_mom [2, n, dim] (None without v_traj) from ITS OWN trajectories by the
    fp32 recurrences of the contract."""
    mean, m2 = welford(traj, h)
    e_mean, e_m2 = welford(e_traj, h)
    mom = torch.stack((mean[0], m2[0], mean[1], m2[1]))
    e_mom = torch.stack((e_mean[0], e_m2[0], e_mean[1], e_m2[1]))
    return mom, e_mom, (None if v_traj is None else v2_mean(v_traj, h))
