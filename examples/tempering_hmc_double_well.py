"""Replica-exchange HMC on a double well whose barrier plain HMC does not cross.

4096 chains start in the left well of DoubleWellModel(barrier_height=10).  After 400 transitions (step size 0.05, five
leapfrog steps) plain HMC still has (almost) all of them there; the tempered ladder (temperatures 1, 2, 4, 8, a swap event
after every transition) has the target slot split evenly between the wells -- and, unlike the tempered Langevin ladder, every
slot is Metropolis-corrected, so the target slot samples exp(-E) without a step-size bias.  On a CUDA device each sampler
call is one fused HIP kernel launch."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

from torchebm_amd.core import DoubleWellModel
from torchebm_amd.samplers import HamiltonianMonteCarlo, ReplicaExchangeHMC

SMOKE = os.getenv("TORCHEBM_SMOKE") == "1"
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
device_name = torch.cuda.get_device_name(0) if device.type == "cuda" else "cpu"

energy = DoubleWellModel(barrier_height=10.0, device=device)
n, k = (128, 40) if SMOKE else (4096, 400)
start = torch.full((n, 2), -1.0, device=device)

plain = HamiltonianMonteCarlo(energy, step_size=0.05, n_leapfrog_steps=5, device=device).sample(x=start, n_steps=k)
tempered = ReplicaExchangeHMC(energy, step_size=0.05, n_leapfrog_steps=5, temperatures=(1.0, 2.0, 4.0, 8.0), swap_every=1,
                              device=device)
ladders, diag = tempered.sample(x=start, n_steps=k, return_replicas=True, return_diagnostics=True)

print(f"device={device} ({device_name})  {n} chains, {k} transitions, all started at x0 = -1")
print(f"plain HMC:         fraction with x0 > 0 = {(plain[:, 0] > 0).float().mean().item():.3f}")
print(f"replica exchange:  fraction with x0 > 0 = {(ladders[:, 0, 0] > 0).float().mean().item():.3f}  (target slot)")
print("per-slot fraction:", [round((ladders[:, r, 0] > 0).float().mean().item(), 3) for r in range(ladders.shape[1])])
print("MH acceptance of the slots:", [round(v, 3) for v in diag["acceptance_rate"].tolist()])
print("swap acceptance of the adjacent pairs:", [round(v, 3) for v in diag["swap_acceptance"].tolist()])
