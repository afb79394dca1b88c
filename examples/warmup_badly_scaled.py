"""Warm a sampler up on a badly scaled target: windows of step-size adaptation and of mass estimation, then sample.

The target is a Gaussian with sigma = (1, 0.1, 0.01).  At unit mass the leapfrog step is bound by the narrowest coordinate
(eps < 2 * 0.01) while the widest needs a hundred times that to move.  GeneralizedHMC(friction=inf) -- plain HMC -- starts from
unit mass and eps = 0.005; warmup() alternates windows that adapt the step size by dual averaging (every chain its own, pooled by
the median) with an estimate of the diagonal mass from the variance of the chains' positions, as Stan's and NumPyro's warm-up
does, and ends on a step-size window under the final mass.  With m_j sigma_j^2 = 1 in every coordinate the target is a unit
Gaussian in the scaled coordinates and the step size grows a hundredfold.

    python examples/warmup_badly_scaled.py

On a CUDA device every window is one fused launch, and so is the production run."""

import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torchebm_amd as ta  # noqa: E402
from torchebm_amd.samplers import GeneralizedHMC  # noqa: E402

SMOKE = os.environ.get("TORCHEBM_SMOKE") == "1"
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
SIGMA, EPS0, L, TARGET = (1.0, 0.1, 0.01), 0.005, 4, 0.8
N, WINDOWS, FINAL, STEPS = (256, (20, 20, 30), 20, 20) if SMOKE else (4096, (50, 50, 100), 50, 100)

sigma = torch.tensor(SIGMA)
energy = ta.GaussianModel(torch.zeros(3), torch.diag(sigma**2), device=device)
sampler = GeneralizedHMC(energy, step_size=EPS0, n_leapfrog_steps=L, friction=math.inf, device=device)
start = (sigma * torch.randn(N, 3, generator=torch.Generator().manual_seed(0))).to(device)
g = torch.Generator(device=device).manual_seed(1)

print(f"device: {device}  chains: {N} x 3  sigma = {SIGMA}  windows: {WINDOWS} + {FINAL} transitions from eps = {EPS0}, L = {L}")
w = sampler.warmup(x=start, windows=WINDOWS, final_steps=FINAL, target_accept=TARGET, generator=g)
unit = [1.0, 1.0, 1.0]
for i, (eps, acc) in enumerate(zip(w.step_sizes, w.acceptances)):
    mass = unit if i == 0 else w.masses[i - 1].cpu()
    scaled = [round(float(m) * s * s, 3) for m, s in zip(mass, SIGMA)]
    kind = "terminal" if i == len(WINDOWS) else f"window {i}"
    print(f"{kind:>9}: ran under m sigma^2 = {scaled}, adapted eps = {float(eps):.4f}, acceptance while adapting {float(acc):.3f}")
assert sampler.get_scheduled_value("step_size") == float(w.step_size) and torch.equal(sampler.mass, w.mass)

x, diag = sampler.sample(x=w.x, n_steps=STEPS, return_diagnostics=True, generator=g)
print(f"production: eps = {float(w.step_size):.4f} ({float(w.step_size) / EPS0:.0f} x the start), acceptance "
      f"{diag['acceptance_rate'].mean().item():.3f} over {STEPS} transitions; std of x = "
      f"{[round(v, 4) for v in x.std(0).tolist()]}")
