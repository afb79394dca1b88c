"""Replica-exchange Langevin on a double well whose barrier plain Langevin does not cross.

4096 chains start in the left well of DoubleWellModel(barrier_height=10).  After 2000 steps plain Langevin still has
(almost) all of them there; the tempered ladder (temperatures 1, 2, 4, 8, a swap event every 5 steps) has the target
slot split evenly between the wells.  On a CUDA device each sampler call is one fused HIP kernel launch."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

from torchebm_amd.core import DoubleWellModel
from torchebm_amd.samplers import LangevinDynamics, ReplicaExchangeLangevin

SMOKE = os.getenv("TORCHEBM_SMOKE") == "1"
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")

energy = DoubleWellModel(barrier_height=10.0, device=device)
n, k = (128, 100) if SMOKE else (4096, 2000)
start = torch.full((n, 2), -1.0, device=device)

plain = LangevinDynamics(energy, step_size=0.004, device=device).sample(x=start, n_steps=k)
tempered = ReplicaExchangeLangevin(energy, step_size=0.004, temperatures=(1.0, 2.0, 4.0, 8.0), swap_every=5, device=device)
ladders, diag = tempered.sample(x=start, n_steps=k, return_replicas=True, return_diagnostics=True)

print(f"device={device}  {n} chains, {k} steps, all started at x0 = -1")
print(f"plain Langevin:    fraction with x0 > 0 = {(plain[:, 0] > 0).float().mean().item():.3f}")
print(f"replica exchange:  fraction with x0 > 0 = {(ladders[:, 0, 0] > 0).float().mean().item():.3f}  (target slot)")
print("per-slot fraction:", [round((ladders[:, r, 0] > 0).float().mean().item(), 3) for r in range(ladders.shape[1])])
print("swap acceptance of the adjacent pairs:", [round(v, 3) for v in diag["swap_acceptance"].tolist()])
