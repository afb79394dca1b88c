"""Are k = 20 Langevin steps from the replay buffer enough?  Split R-hat and ESS of contrastive divergence's own negative chains.

An `MLPEnergy(2)` is trained on two-moons by persistent contrastive divergence, its negatives drawn by `LangevinDynamics` with
k = 20 steps per training step from a replay buffer (the package's default training sampler, BASELINE config 5).  Afterwards the
same sampler continues chains from the buffer with `sample_moments(energy=True)`, once for the k = 20 steps training uses and once
for k = 200: `ChainMoments` forms split R-hat, a between-sequence effective sample size and the same for the energy from a time
average and a sum of squared deviations per chain and half of the run.  A split R-hat near 1 over 20 steps says the two halves of
a chain and the chains among each other agree already -- the buffer holds samples of the model, and 20 steps keep them there;
well above 1 it says the 20 steps are a transient and the negatives describe the buffer's past, not the model.

With `sampler.fused_mlp_moments = True` on a CUDA device each `sample_moments` call -- the Philox draws, k evaluations on the matrix
cores (one more for the energies) and the accumulators -- is ONE launch of `ebm_chain_moments_mlp_f32`
(docs/design/langevin_moments_mlp.md); on the CPU the same call takes the eager route."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

from torchebm_amd.core import MLPEnergy
from torchebm_amd.losses import ContrastiveDivergence
from torchebm_amd.samplers import LangevinDynamics
from torchebm_amd.utils.synthetic import two_moons

SMOKE = os.getenv("TORCHEBM_SMOKE") == "1"
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
device_name = torch.cuda.get_device_name(0) if device.type == "cuda" else "cpu"
# the CPU runs a reduced size: the eager route is one autograd pass per step and chain batch
TRAIN_STEPS, N_CHAINS, HIDDEN = (10, 64, 64) if SMOKE else ((600, 4096, 128) if device.type == "cuda" else (150, 512, 64))
K_TRAIN, K_LONG = 20, 200

torch.manual_seed(0)
data = two_moons(n_samples=3000, noise=0.05, seed=0, device=device)
energy = MLPEnergy(2, HIDDEN, device=device)
sampler = LangevinDynamics(model=energy, step_size=0.01, noise_scale=1.0, device=device)
sampler.fused_mlp_moments = True  # one ebm_chain_moments_mlp_f32 launch per sample_moments() on a CUDA device; the eager route elsewhere
pcd = ContrastiveDivergence(model=energy, sampler=sampler, k_steps=K_TRAIN, persistent=True, buffer_size=8192, device=device)
opt = torch.optim.Adam(energy.parameters(), lr=1e-3)

for step in range(TRAIN_STEPS):
    batch = data[torch.randint(len(data), (256,), device=device)]
    loss, negatives = pcd(batch)
    opt.zero_grad()
    loss.backward()
    opt.step()
print(f"device={device} ({device_name})  trained {TRAIN_STEPS} PCD steps, final loss {loss.item():+.3f}")

buffer = pcd.replay_buffer.detach()
start = buffer[torch.randperm(len(buffer), device=buffer.device)[:N_CHAINS]].to(device)
for k in (K_TRAIN, K_LONG):
    _, m = sampler.sample_moments(x=start, n_steps=k, energy=True, generator=torch.Generator(device=device).manual_seed(1))
    print(f"k = {k:3d} Langevin steps from the replay buffer, {N_CHAINS} chains:  max split R-hat = {float(m.rhat.max()):.3f}, "
          f"min ESS = {float(m.ess.min()):.0f} of {2 * N_CHAINS * m.half_len} counted states, energy R-hat = {float(m.energy_rhat):.3f}")
print("R-hat near 1 at k = 20: the buffer's chains agree with each other and with themselves over the steps training takes; "
      "well above 1: the 20 steps are a transient -- compare the k = 200 line.")
route = sampler._route(start, {})[0]
print("route", route, "+ fused_mlp_moments" if route == "fused" else "")
