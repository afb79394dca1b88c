"""Running moments of the Euler-Maruyama walk on the MLP energy (include/ebm_hip.h, ebm_chain_moments_mlp_f32): the cases the tests
run and their restatements, composed from what exists -- the networks and the autograd oracle of kinetic_mlp_cases.py, the
Euler-Maruyama restatement, the Welford recurrence and the reciprocal table of moments_cases.py, the shapes of
kinetic_moments_mlp_cases.py.  Shared by test_langevin_moments_mlp.py (CPU tier) and test_langevin_moments_mlp_gpu.py; it never
calls the package's samplers."""

import copy
import functools

import torch

import kinetic_mlp_cases
from kinetic_mlp_cases import CpuMlpEnergy
from kinetic_moments_mlp_cases import GHMC_CASES
from moments_cases import recip_table, restate_langevin, split, welford  # noqa: F401

ETA, SIGMA = 0.05, 1.0

# (in_dim, hidden, n, k, burn_in): the 13 shapes of kinetic_moments_mlp_cases.GHMC_CASES -- every (HT, DT), the per-element Philox
# path (dim % 4 != 0) and the per-quad one, a partial wave (37 = 32 + 5 chains), several workgroups and a tail (257, 129) --;
# (k, burn_in) = (4, 0), (7, 3), (11, 3) down the list: the shortest halves h = 2, and a burn-in in front of h = 2 and h = 4.
_RUNS = [(4, 0), (7, 3), (11, 3)]
CASES = [(c[0], c[1], c[2], *_RUNS[i % 3]) for i, c in enumerate(GHMC_CASES)]


def coefficients(eta=ETA, sigma=SIGMA):
    """(eta, sqrt_eta, noise_coef) as restate_langevin forms them, in double; the entry takes them as fp32."""
    return eta, eta**0.5, (2.0 * sigma**2) ** 0.5


@functools.lru_cache(maxsize=None)
def case(in_dim, hidden, n, k, burn_in):
    """Inputs and both restatements (moments_cases.restate_langevin on the network of kinetic_mlp_cases.net) of a case: x [n, dim],
    traj [n, 2 h, dim], e_traj [n, 2 h].  Computed once per session and shared (read-only)."""
    cpu = kinetic_mlp_cases.net(in_dim, hidden)
    g = torch.Generator().manual_seed(7000 + in_dim + n)
    x0 = torch.randn(n, in_dim, generator=g)
    noise = torch.randn(k, n, in_dim, generator=g)
    ref32 = restate_langevin(CpuMlpEnergy(cpu), x0, noise, ETA, SIGMA, burn_in, torch.float32)
    ref64 = restate_langevin(CpuMlpEnergy(copy.deepcopy(cpu).double()), x0, noise, ETA, SIGMA, burn_in, torch.float64)
    return {"cpu": cpu, "x0": x0, "noise": noise, "ref32": ref32, "ref64": ref64, "shape": (n, in_dim), "k": k, "burn_in": burn_in,
            "half": split(k, burn_in)}


def restatement_errors(c, keys=("x", "traj", "e_traj")):
    """{key: (fp32 restatement's max error against fp64, max |fp64|)} of a case."""
    out = {}
    for key in keys:
        ref = c["ref64"][key]
        out[key] = ((c["ref32"][key].double() - ref).abs().max().item(), ref.abs().max().item())
    return out


def moments_of(traj, e_traj, h):
    """The entry's mom [4, n, dim] and e_mom [4, n] from ITS OWN trajectories by the fp32 recurrence of the contract."""
    mean, m2 = welford(traj, h)
    e_mean, e_m2 = welford(e_traj, h)
    return torch.stack((mean[0], m2[0], mean[1], m2[1])), torch.stack((e_mean[0], e_m2[0], e_mean[1], e_m2[1]))
