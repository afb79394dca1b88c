"""Replica-exchange Langevin on a TRAINED energy with two modes that plain Langevin dynamics does not travel between.

A small `MLPEnergy(2, 64)` is trained by persistent contrastive divergence on two well separated Gaussian blobs.  Then every chain
starts in the left blob.  Plain Langevin dynamics -- the sampler the training itself runs -- leaves most of them there; the
tempered ladder (temperatures 1, 2, 4, 8, a swap event every 5 steps) carries crossings of the hot slots down to the target slot.
How evenly the target slot ends up split depends on how well the short training run balanced the two modes -- the point is the
difference between the two samplers (on an MI355X: 0.04 of the chains in the other blob after plain Langevin dynamics, 0.38
after the ladder).

With `sampler.fused_mlp_ladder = True` and the packaged `MLPEnergy` on a CUDA device the whole `sample()` call -- every slot's
draws, one evaluation on the matrix cores per step, the swap events on that evaluation's energies, the counters -- is ONE launch of
`ebm_tempering_mlp_chain_f32` (docs/design/tempering_mlp.md); on the CPU the same sampler takes its eager route."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

from torchebm_amd.core import MLPEnergy
from torchebm_amd.losses import ContrastiveDivergence
from torchebm_amd.samplers import LangevinDynamics, ReplicaExchangeLangevin

SMOKE = os.getenv("TORCHEBM_SMOKE") == "1"
TRAIN_STEPS, N_CHAINS, N_STEPS = (20, 64, 20) if SMOKE else (800, 2048, 1000)
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
plain = LangevinDynamics(energy, step_size=0.01, noise_scale=1.0, device=device).sample(x=start, n_steps=N_STEPS)
tempered = ReplicaExchangeLangevin(energy, step_size=0.01, noise_scale=1.0, temperatures=(1.0, 2.0, 4.0, 8.0), swap_every=5, device=device)
tempered.fused_mlp_ladder = True  # one ebm_tempering_mlp_chain_f32 launch per sample() on a CUDA device; the eager route elsewhere
ladders, diag = tempered.sample(x=start, n_steps=N_STEPS, return_replicas=True, return_diagnostics=True)

print(f"device={device} ({device_name})  {N_CHAINS} chains, {N_STEPS} steps, all started in the blob at x0 = {centres[0, 0].item():+.2f}")
print(f"plain Langevin:    share of chains in the other blob (x0 > 0) = {(plain[:, 0] > 0).float().mean().item():.3f}")
print(f"replica exchange:  share of chains in the other blob (x0 > 0) = {(ladders[:, 0, 0] > 0).float().mean().item():.3f}  (target slot)")
print("per-slot share:", [round((ladders[:, r, 0] > 0).float().mean().item(), 3) for r in range(ladders.shape[1])])
print("swap acceptance of the adjacent pairs:", [round(v, 3) for v in diag["swap_acceptance"].tolist()])
print("route", tempered._route(ladders)[0])
