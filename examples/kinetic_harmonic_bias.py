"""Step-size bias on a harmonic well: underdamped Langevin (BAOAB) beside Euler-Maruyama.

On E(x) = k x^2 / 2 the stationary variance is 1 / k.  Euler-Maruyama with step eta samples a variance that is too large by
1 / (1 - eta k / 2); BAOAB's position marginal is exact for every stable step size.  With k = 4, BAOAB at h = 0.3 and
Euler-Maruyama at the matching step eta = h^2 / 2 = 0.045 this prints var(x) * k of about 1.00 against about 1.10 -- at one
gradient evaluation per step for both.  The velocities show the step size instead: var(v) = 1 - h^2 k / 4 = 0.91.

    python examples/kinetic_harmonic_bias.py

On a CUDA device each sampler call is one fused launch."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchebm_amd import HarmonicModel  # noqa: E402
from torchebm_amd.samplers import LangevinDynamics, UnderdampedLangevin  # noqa: E402

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
K_SPRING, H, N, DIM, STEPS = 4.0, 0.3, 16384, 4, 400

print(f"device: {device}  chains: {N} x {DIM}  steps: {STEPS}")
energy = HarmonicModel(k=K_SPRING, device=device)
start = 0.5 * torch.randn(N, DIM, device=device, generator=torch.Generator(device=device).manual_seed(0))

kinetic = UnderdampedLangevin(energy, step_size=H, friction=1.0, temperature=1.0, device=device)
x, diag = kinetic.sample(x=start, n_steps=STEPS, return_diagnostics=True, generator=torch.Generator(device=device).manual_seed(1))
print(f"UnderdampedLangevin(step_size={H}):      var(x) * k = {x.var().item() * K_SPRING:.3f}   "
      f"kinetic temperature = {diag['kinetic_temperature'].item():.3f} (1 - h^2 k / 4 = {1 - H * H * K_SPRING / 4:.2f})")

plain = LangevinDynamics(energy, step_size=H * H / 2, device=device)
y = plain.sample(x=start, n_steps=STEPS, generator=torch.Generator(device=device).manual_seed(1))
print(f"LangevinDynamics(step_size={H * H / 2:.3f}):       var(x) * k = {y.var().item() * K_SPRING:.3f}   "
      f"(1 / (1 - eta k / 2) = {1 / (1 - H * H / 2 * K_SPRING / 2):.3f})")
