"""Persistent contrastive divergence on two-moons with Metropolis-corrected negatives: the loop of pcd_kinetic_two_moons.py
with `GeneralizedHMC` drawing the negatives instead of `UnderdampedLangevin`, so no step-size bias is left in them.

With `sampler.fused_mlp = True` and the packaged `MLPEnergy` on a CUDA device all k transitions of a `sample()` call -- the start
velocities, the partial refreshes, L + 1 evaluations on the matrix cores per trajectory, the accept decisions, the flips, the
Philox draws -- are ONE launch of `ebm_ghmc_mlp_chain_f32` (docs/design/ghmc_mlp.md); on the CPU the same sampler takes its
eager route.  Each `sample()` call draws fresh velocities from N(0, T I): the replay buffer keeps positions only."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

from torchebm_amd.core import MLPEnergy
from torchebm_amd.losses import ContrastiveDivergence
from torchebm_amd.samplers import GeneralizedHMC
from torchebm_amd.utils.synthetic import two_moons

SMOKE = os.getenv("TORCHEBM_SMOKE") == "1"
N_STEPS = 20 if SMOKE else 1000
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")

torch.manual_seed(0)
data = two_moons(n_samples=3000, noise=0.05, seed=0, device=device)
energy = MLPEnergy(2, device=device)
# eps = 0.15, L = 2: a trajectory as long as a BAOAB step of pcd_kinetic_two_moons.py; gamma = 2 keeps half the velocity per transition
sampler = GeneralizedHMC(model=energy, step_size=0.15, n_leapfrog_steps=2, friction=2.0, temperature=1.0, device=device)
sampler.fused_mlp = True  # one ebm_ghmc_mlp_chain_f32 launch per sample() on a CUDA device; the eager route elsewhere
pcd = ContrastiveDivergence(model=energy, sampler=sampler, k_steps=10, persistent=True, buffer_size=8192, device=device)
opt = torch.optim.Adam(energy.parameters(), lr=1e-3)

for step in range(N_STEPS):
    batch = data[torch.randint(len(data), (256,), device=device)]
    loss, negatives = pcd(batch)
    opt.zero_grad()
    loss.backward()
    opt.step()
    if step % 200 == 0 or step == N_STEPS - 1:
        with torch.no_grad():
            gap = energy(negatives).mean() - energy(batch).mean()
        print(f"step {step:4d}  loss {loss.item():+.3f}  E(neg) - E(data) = {gap.item():+.3f}")
_, diag = sampler.sample(x=negatives, n_steps=10, return_diagnostics=True)
print(f"acceptance of the last negatives' chains: {diag['acceptance_rate'].mean().item():.3f}")
print("route", sampler._route(batch)[0], "-- done on", device)
