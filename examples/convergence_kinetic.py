"""Does the inertia pay?  Split R-hat and ESS of BAOAB against Euler-Maruyama from per-chain running moments, and the step-size
error read off the kinetic temperature.

Chains of DoubleWellModel(barrier_height=2) at dim 2 start half in each well and are given the same number of gradient
evaluations under overdamped Langevin (Euler-Maruyama) and under underdamped Langevin (BAOAB), each at a step size its
stability allows.  `sample_moments` keeps a time average and a sum of squared deviations per chain, coordinate and half of the
run -- no trajectory -- and ChainMoments turns them into split R-hat and a between-sequence effective sample size.  BAOAB also
keeps the running mean of v^2: on a quadratic well it is T (1 - h^2 E'' / 4), so its distance from T shows what the step size
costs.  On a CUDA device each `sample_moments` call is one fused HIP kernel launch."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

from torchebm_amd.core import DoubleWellModel
from torchebm_amd.samplers import LangevinDynamics, UnderdampedLangevin

SMOKE = os.getenv("TORCHEBM_SMOKE") == "1"
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")

energy = DoubleWellModel(barrier_height=2.0, device=device)
n, k, burn_in = (128, 200, 40) if SMOKE else (2048, 2000, 400)
start = torch.ones(n, 2, device=device)
start[: n // 2] = -1.0

_, em = LangevinDynamics(energy, step_size=0.01, device=device).sample_moments(x=start, n_steps=k, burn_in=burn_in)
runs = {}
for h in (0.05, 0.2):
    _, runs[h] = UnderdampedLangevin(energy, step_size=h, friction=1.0, device=device).sample_moments(x=start, n_steps=k, burn_in=burn_in)
baoab = runs[0.2]

fmt = lambda t, d=2: [round(v, d) for v in t.tolist()]  # noqa: E731
print(f"device={device}  {n} chains, {k} steps ({burn_in} burnt), half started in each well of a barrier-2 double well.")
print(f"Euler-Maruyama, step 0.01: split R-hat = {fmt(em.rhat, 3)}, ESS = {fmt(em.ess, 0)} of {2 * n * em.half_len} counted states "
      f"(+- {100 * em.ess_rel_stderr:.0f} %).  BAOAB, step 0.2, the same number of gradients: split R-hat = {fmt(baoab.rhat, 3)}, "
      f"ESS = {fmt(baoab.ess, 0)}.")
print("Time-averaged kinetic temperature (T = 1): "
      + ", ".join(f"step {h}: {fmt(m.kinetic_temperature, 3)}" for h, m in runs.items())
      + " -- the larger step runs the velocities colder, the price of the discretisation.")
