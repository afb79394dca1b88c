"""Momentum that persists: generalized HMC beside HamiltonianMonteCarlo at one leapfrog step per transition.

An ill-conditioned Gaussian: coordinate 0 has standard deviation 1, coordinate 1 has 0.1 and caps the step size at eps = 0.1.
HamiltonianMonteCarlo with L = 1 (MALA) draws a fresh momentum at every transition: coordinate 0 moves by about eps per
transition in a random direction, and after THIN = 50 transitions it is still where it was -- a lag-1 autocorrelation of the kept
states near (1 - eps^2 / 2)^50 = 0.78.  GeneralizedHMC with the same eps, the same L -- the same number of gradient evaluations
-- and friction 1 keeps exp(-0.1) = 0.90 of its velocity per transition: it crosses the slow direction and the same
autocorrelation is near zero.  Both are Metropolis-adjusted: the variance of coordinate 0 is 1 for both.

    python examples/ghmc_persistence.py

On a CUDA device each sampler call is one fused launch."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchebm_amd import GaussianModel  # noqa: E402
from torchebm_amd.samplers import GeneralizedHMC, HamiltonianMonteCarlo  # noqa: E402

SMOKE = os.environ.get("TORCHEBM_SMOKE") == "1"
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
EPS, THIN = 0.1, 50
N, STEPS = (256, 400) if SMOKE else (4096, 2000)

print(f"device: {device}  chains: {N} x 2  transitions: {STEPS}, kept every {THIN}  (one gradient evaluation per transition for both)")
sigma = torch.tensor([1.0, 0.1])
energy = GaussianModel(torch.zeros(2), torch.diag(sigma**2), device=device)
start = (sigma * torch.randn(N, 2, generator=torch.Generator().manual_seed(0))).to(device)


def lag1(traj):
    """Autocorrelation of coordinate 0 between consecutive kept states, pooled over the chains."""
    a, b = traj[:, :-1, 0].double().flatten(), traj[:, 1:, 0].double().flatten()
    return ((a - a.mean()) * (b - b.mean())).mean().item() / (a.std(unbiased=False) * b.std(unbiased=False)).item()


hmc = HamiltonianMonteCarlo(energy, step_size=EPS, n_leapfrog_steps=1, device=device)
traj = hmc.sample(x=start, n_steps=STEPS, thin=THIN, return_trajectory=True, generator=torch.Generator(device=device).manual_seed(1))
print(f"HamiltonianMonteCarlo(L=1):            lag-1 autocorrelation of the slow coordinate = {lag1(traj):+.3f}   "
      f"var = {traj[:, -1, 0].var().item():.3f}")

ghmc = GeneralizedHMC(energy, step_size=EPS, n_leapfrog_steps=1, friction=1.0, device=device)
traj, diag = ghmc.sample(x=start, n_steps=STEPS, thin=THIN, return_trajectory=True, return_diagnostics=True,
                         generator=torch.Generator(device=device).manual_seed(1))
print(f"GeneralizedHMC(L=1, friction=1):       lag-1 autocorrelation of the slow coordinate = {lag1(traj):+.3f}   "
      f"var = {traj[:, -1, 0].var().item():.3f}   acceptance = {diag['acceptance_rate'].mean().item():.3f}")
