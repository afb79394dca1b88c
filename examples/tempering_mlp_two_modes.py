"""Replica-exchange HMC on a TRAINED energy with two modes that plain HMC does not travel between.

A small `MLPEnergy(2, 64)` is trained by persistent contrastive divergence on two well separated Gaussian blobs.  Then every chain
starts in the left blob.  Plain HMC leaves (almost) all of them there; the tempered ladder (temperatures 1, 2, 4, 8, a swap event
after every transition) carries crossings of the hot slots down to the target slot.  How evenly the target slot ends up split
depends on how well the short training run balanced the two modes -- the point is the difference between the two samplers (on the
CPU: about a tenth of the chains in the other blob after plain HMC, about half after the ladder).

With `sampler.fused_mlp = True` and the packaged `MLPEnergy` on a CUDA device the whole `sample()` call -- every slot's draws,
L + 1 evaluations on the matrix cores per trajectory, the accept decisions, the swap events, the counters -- is ONE launch of
`ebm_tempering_hmc_mlp_chain_f32` (docs/design/tempering_hmc_mlp.md); on the CPU the same sampler takes its eager route."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

from torchebm_amd.core import MLPEnergy
from torchebm_amd.losses import ContrastiveDivergence
from torchebm_amd.samplers import HamiltonianMonteCarlo, LangevinDynamics, ReplicaExchangeHMC

SMOKE = os.getenv("TORCHEBM_SMOKE") == "1"
TRAIN_STEPS, N_CHAINS, N_TRANSITIONS = (20, 64, 10) if SMOKE else (800, 2048, 300)
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
device_name = torch.cuda.get_device_name(0) if device.type == "cuda" else "cpu"

torch.manual_seed(0)
centres = torch.tensor([[-1.75, 0.0], [1.75, 0.0]], device=device)
data = centres[torch.randint(2, (4000,), device=device)] + 0.3 * torch.randn(4000, 2, device=device)

energy = MLPEnergy(2, 64, device=device)
trainer = LangevinDynamics(model=energy, step_size=0.05, noise_scale=1.0, device=device)
pcd = ContrastiveDivergence(model=energy, sampler=trainer, k_steps=10, persistent=True, buffer_size=4096, energy_reg_weight=0.1, device=device)
opt = torch.optim.Adam(energy.parameters(), lr=1e-3)
for step in range(TRAIN_STEPS):
    batch = data[torch.randint(len(data), (256,), device=device)]
    loss, negatives = pcd(batch)
    opt.zero_grad()
    loss.backward()
    opt.step()
    if step % 500 == 0 or step == TRAIN_STEPS - 1:
        print(f"step {step:4d}  loss {loss.item():+.3f}")

start = centres[0] + 0.3 * torch.randn(N_CHAINS, 2, device=device)  # every chain in the left blob
plain = HamiltonianMonteCarlo(energy, step_size=0.1, n_leapfrog_steps=5, device=device).sample(x=start, n_steps=N_TRANSITIONS)
tempered = ReplicaExchangeHMC(energy, step_size=0.1, n_leapfrog_steps=5, temperatures=(1.0, 2.0, 4.0, 8.0), swap_every=1, device=device)
tempered.fused_mlp = True  # one ebm_tempering_hmc_mlp_chain_f32 launch per sample() on a CUDA device; the eager route elsewhere
ladders, diag = tempered.sample(x=start, n_steps=N_TRANSITIONS, return_replicas=True, return_diagnostics=True)

print(f"device={device} ({device_name})  {N_CHAINS} chains, {N_TRANSITIONS} transitions, all started in the blob at x0 = {centres[0, 0].item():+.2f}")
print(f"plain HMC:         share of chains in the other blob (x0 > 0) = {(plain[:, 0] > 0).float().mean().item():.3f}")
print(f"replica exchange:  share of chains in the other blob (x0 > 0) = {(ladders[:, 0, 0] > 0).float().mean().item():.3f}  (target slot)")
print("per-slot share:", [round((ladders[:, r, 0] > 0).float().mean().item(), 3) for r in range(ladders.shape[1])])
print("MH acceptance of the slots:", [round(v, 3) for v in diag["acceptance_rate"].tolist()])
print("swap acceptance of the adjacent pairs:", [round(v, 3) for v in diag["swap_acceptance"].tolist()])
print("route", tempered._route(ladders)[0])
