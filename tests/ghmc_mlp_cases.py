"""Generalized HMC on the MLP energy (include/ebm_hip.h, ebm_ghmc_mlp_chain_f32): the restatement of ghmc_cases.py with energy
and gradient from autograd on the network, the networks, the cases the tests run, and their inputs.  Shared by test_ghmc_mlp.py
(CPU tier) and test_ghmc_mlp_gpu.py; it never calls the package's sampler."""

import copy
import functools
import math

import torch

from ghmc_cases import MARGIN_BAR, constants, restate  # noqa: F401
from kinetic_mlp_cases import CpuMlpEnergy
from kinetic_mlp_cases import net as _flat_net

GAMMA, TEMP, EPS = 1.5, 0.8, 1.0
SHARPEN = 2.5  # on top of kinetic_mlp_cases.net's 1.2: 3 x the default initialisation
MAX_SEEDS = 20
MIN_DECISIONS = 3  # accepted and rejected decisions every case must hold in fp64

# (in_dim, hidden, n, n_mh, thin, L): every (HT, DT) -- hidden 64 / 128 at dims 1 .. 32, 33 .. 64, 65 .. 96, 97 .. 128 -- the
# per-element Philox path (dim % 4 != 0: 1, 2, 5, 30, 33, 65) and the per-quad one, partial waves (37 = 32 + 5 chains), several
# workgroups and a tail (257 = 2 x 128 + 1), (n_mh, thin) = (1, 1) one transition, (4, 2), (6, 3), L = 1 (a trajectory of its two
# half kicks) and L = 3.
CASES = [
    (2, 64, 257, 6, 3, 1),
    (1, 64, 37, 4, 2, 3),
    (5, 128, 37, 4, 2, 1),
    (30, 128, 257, 1, 1, 3),
    (32, 64, 129, 6, 3, 1),
    (33, 128, 37, 4, 2, 3),
    (40, 64, 37, 4, 2, 1),
    (64, 128, 129, 4, 2, 1),
    (65, 64, 37, 1, 1, 3),
    (96, 128, 37, 4, 2, 1),
    (100, 64, 129, 4, 2, 3),
    (128, 64, 37, 4, 2, 1),
    (128, 128, 37, 6, 3, 3),
]
INF_CASE = (33, 128, 37, 4, 2, 3)  # run once more with gamma = inf: c1 = 0, c2 = sqrt_temp, the HMC transition
# the step size of a case, where it is not EPS (a case that misses the conditions below changes its eps, never the bars)
CASE_EPS = {}


@functools.lru_cache(maxsize=None)
def net(in_dim, hidden):
    """kinetic_mlp_cases.net on a deep copy with every parameter x 2.5 more: the x 1.2 networks are too flat for this sampler
    (at eps <= 0.6 they reject nothing), and the flip would go untested."""
    cpu = copy.deepcopy(_flat_net(in_dim, hidden))
    with torch.no_grad():
        for p in cpu.parameters():
            p.mul_(SHARPEN)
    return cpu


def draw_inputs(seed, in_dim, n, n_mh):
    g = torch.Generator().manual_seed(7300 + seed + in_dim + n)
    x0 = torch.randn(n, in_dim, generator=g)
    v0 = math.sqrt(TEMP) * torch.randn(n, in_dim, generator=g)
    return x0, v0, torch.randn(n_mh, n, in_dim, generator=g), torch.rand(n_mh, n, generator=g)


@functools.lru_cache(maxsize=None)
def case(in_dim, hidden, n, n_mh, thin, L, gamma=GAMMA):
    """Inputs and both restatements of a case, computed once per session and shared (read-only).  The seed is the first whose
    fp64 restatement has no decision closer than MARGIN_BAR to its threshold and whose fp32 restatement decides alike; "found"
    says whether one of the first MAX_SEEDS did."""
    cpu = net(in_dim, hidden)
    e32, e64 = CpuMlpEnergy(cpu), CpuMlpEnergy(copy.deepcopy(cpu).double())
    eps = CASE_EPS.get((in_dim, hidden, n, n_mh, thin, L), EPS)
    found = False
    for seed in range(MAX_SEEDS):
        x0, v0, z, u = draw_inputs(seed, in_dim, n, n_mh)
        ref64 = restate(e64, x0, v0, z, u, eps, L, gamma, TEMP, torch.float64, thin)
        ref32 = None
        if ref64["margin"] <= MARGIN_BAR:
            continue
        ref32 = restate(e32, x0, v0, z, u, eps, L, gamma, TEMP, torch.float32, thin)
        if torch.equal(ref32["accepted"], ref64["accepted"]):
            found = True
            break
    if ref32 is None:
        ref32 = restate(e32, x0, v0, z, u, eps, L, gamma, TEMP, torch.float32, thin)
    return {"cpu": cpu, "x0": x0, "v0": v0, "z": z, "u": u, "eps": eps, "L": L, "gamma": gamma, "temp": TEMP, "ref32": ref32,
            "ref64": ref64, "seed": seed, "found": found, "shape": (n, in_dim), "n_mh": n_mh, "thin": thin}


def restatement_errors(c):
    """{key: (fp32 restatement's max error against fp64, max |fp64|)} for x, v and traj of a case."""
    out = {}
    for key in ("x", "v", "traj"):
        ref = c["ref64"][key]
        out[key] = ((c["ref32"][key].double() - ref).abs().max().item(), ref.abs().max().item())
    return out
