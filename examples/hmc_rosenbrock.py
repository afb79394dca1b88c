"""HMC on the 2-D Rosenbrock valley (a = 1, b = 100): the whole sample() call is one kernel launch on the GPU."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

from torchebm_amd.core import RosenbrockModel
from torchebm_amd.samplers import HamiltonianMonteCarlo

SMOKE = os.getenv("TORCHEBM_SMOKE") == "1"
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")

energy = RosenbrockModel(a=1.0, b=100.0, device=device)
sampler = HamiltonianMonteCarlo(energy, step_size=0.01, n_leapfrog_steps=20, device=device)
n, steps = (128, 10) if SMOKE else (20_000, 500)
start = torch.randn(n, 2, device=device) * 0.5
x, diag = sampler.sample(x=start, n_steps=steps, thin=max(1, steps // 5), return_diagnostics=True)
print(f"device={device}  acceptance rate per kept step: {[round(v, 3) for v in diag['acceptance_rate'].tolist()]}")
# exp(-E) has its ridge on the parabola x1 = x0^2 around the minimum (1, 1)
print("mean:", [round(v, 3) for v in x.mean(dim=0).tolist()], " mean |x1 - x0^2|:", round((x[:, 1] - x[:, 0] ** 2).abs().mean().item(), 4),
      " mean energy:", round(energy(x).mean().item(), 3))
