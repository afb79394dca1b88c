"""Persistent contrastive divergence on two-moons with a momentum sampler: the loop of pcd_two_moons.py with
`UnderdampedLangevin` (BAOAB) drawing the negatives instead of `LangevinDynamics`.

With `sampler.fused_mlp = True` and the packaged `MLPEnergy` on a CUDA device all k steps of a `sample()` call -- the start
velocities, k + 1 gradient evaluations on the matrix cores, the BAOAB updates, the Philox draws -- are ONE launch of
`ebm_kinetic_mlp_chain_f32` (docs/design/kinetic_mlp.md); on the CPU the same sampler takes its eager route.  Each `sample()` call
draws fresh velocities from N(0, T I): the replay buffer keeps positions only."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

from torchebm_amd.core import MLPEnergy
from torchebm_amd.losses import ContrastiveDivergence
from torchebm_amd.samplers import UnderdampedLangevin
from torchebm_amd.utils.synthetic import two_moons

SMOKE = os.getenv("TORCHEBM_SMOKE") == "1"
N_STEPS = 20 if SMOKE else 1000
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")

torch.manual_seed(0)
data = two_moons(n_samples=3000, noise=0.05, seed=0, device=device)
energy = MLPEnergy(2, device=device)
# h = 0.3 with gamma = 2: the position moves about as far per step as Euler-Maruyama's at step_size = 0.1 (h^2 / 2 ~ eta)
sampler = UnderdampedLangevin(model=energy, step_size=0.3, friction=2.0, temperature=1.0, device=device)
sampler.fused_mlp = True  # one ebm_kinetic_mlp_chain_f32 launch per sample() on a CUDA device; the eager route elsewhere
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
print("route", sampler._route(batch)[0], "-- done on", device)
