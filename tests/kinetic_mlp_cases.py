"""Underdamped Langevin, BAOAB, on the MLP energy (include/ebm_hip.h, ebm_kinetic_mlp_chain_f32): the restatement of
kinetic_cases.py with the gradient from autograd on the network, the networks, the cases the tests run, and their inputs.
Shared by test_kinetic_mlp.py (CPU tier) and test_kinetic_mlp_gpu.py; it never calls the package's sampler."""

import copy
import functools
import math

import torch

import torchebm_amd as ta
from kinetic_cases import constants, restate  # noqa: F401

GAMMA, TEMP, STEP = 1.5, 0.8, 0.2

# (in_dim, hidden, n, k_steps, thin): every (HT, DT) -- hidden 64 / 128 at dims 1 .. 32, 33 .. 64, 65 .. 96, 97 .. 128 -- the
# per-element Philox path (dim % 4 != 0: 1, 2, 5, 30, 33, 65) and the per-quad one, partial waves (37 = 32 + 5 chains),
# several workgroups and a tail (257 = 2 x 128 + 1), (k, thin) = (1, 1) one step, (4, 2), (11, 3) with two steps behind the last
# kept one.
CASES = [
    (2, 64, 257, 11, 3),
    (1, 64, 37, 4, 2),
    (5, 128, 37, 4, 2),
    (30, 128, 257, 1, 1),
    (32, 64, 129, 11, 3),
    (33, 128, 37, 4, 2),
    (40, 64, 37, 4, 2),
    (64, 128, 129, 4, 2),
    (65, 64, 37, 1, 1),
    (96, 128, 37, 4, 2),
    (100, 64, 129, 4, 2),
    (128, 64, 37, 4, 2),
    (128, 128, 37, 11, 3),
]


class CpuMlpEnergy:
    """The oracle interface of kinetic_cases.restate on a CPU network: the gradient from autograd."""

    def __init__(self, model):
        self.model = model

    def energy(self, x):
        return self.model(x).detach()

    def grad(self, x):
        return self.model.gradient(x)


@functools.lru_cache(maxsize=None)
def net(in_dim, hidden):
    """MLPEnergy under manual_seed(10 + in_dim) with every parameter x 1.2 (the networks of test_ais_mlp_gpu.py)."""
    torch.manual_seed(10 + in_dim)
    cpu = ta.MLPEnergy(in_dim, hidden)
    with torch.no_grad():
        for p in cpu.parameters():
            p.mul_(1.2)
    return cpu


@functools.lru_cache(maxsize=None)
def case(in_dim, hidden, n, k, thin):
    """Inputs and both restatements of a case, computed once per session and shared (read-only)."""
    cpu = net(in_dim, hidden)
    g = torch.Generator().manual_seed(7000 + in_dim + n)
    x0 = torch.randn(n, in_dim, generator=g)
    v0 = math.sqrt(TEMP) * torch.randn(n, in_dim, generator=g)
    noise = torch.randn(k, n, in_dim, generator=g)
    ref32 = restate(CpuMlpEnergy(cpu), x0, v0, noise, STEP, GAMMA, TEMP, thin, torch.float32)
    ref64 = restate(CpuMlpEnergy(copy.deepcopy(cpu).double()), x0, v0, noise, STEP, GAMMA, TEMP, thin, torch.float64)
    return {"cpu": cpu, "x0": x0, "v0": v0, "noise": noise, "h": STEP, "ref32": ref32, "ref64": ref64, "shape": (n, in_dim), "k": k,
            "thin": thin}


def restatement_errors(c):
    """{key: (fp32 restatement's max error against fp64, max |fp64|)} for x, v and traj of a case."""
    out = {}
    for key in ("x", "v", "traj"):
        ref = c["ref64"][key]
        out[key] = ((c["ref32"][key].double() - ref).abs().max().item(), ref.abs().max().item())
    return out
