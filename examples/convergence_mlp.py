"""Has a run on a TRAINED energy converged?  Split R-hat and ESS of generalized HMC on an MLPEnergy from per-chain running moments.

A small `MLPEnergy(2, 64)` is trained by persistent contrastive divergence on the two well separated Gaussian blobs of
examples/tempering_mlp_two_modes.py.  Every chain starts in one of its modes (half of them in each) and generalized HMC does not
carry it across in the time given: the chains disagree about the first coordinate, and split R-hat, formed by `ChainMoments` from a
time average and a sum of squared deviations per chain and half of the run, is well above 1 -- the alarm.  On a unimodal network
of the same shape (one whose energy grows in every direction: first-layer directions around the circle, positive weights above)
the same sampler reports R-hat near 1.

With `sampler.fused_mlp = True` and `sampler.fused_mlp_moments = True` on a CUDA device each `sample_moments` call -- the draws,
L + 1 evaluations on the matrix cores per transition, the accept decisions and the accumulators -- is ONE launch of
`ebm_kinetic_moments_mlp_f32` (docs/design/kinetic_moments_mlp.md), the walk that `sample()` runs under `fused_mlp`; on the CPU the
same call takes the eager route."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

from torchebm_amd.core import MLPEnergy
from torchebm_amd.losses import ContrastiveDivergence
from torchebm_amd.samplers import GeneralizedHMC, LangevinDynamics

SMOKE = os.getenv("TORCHEBM_SMOKE") == "1"
TRAIN_STEPS, N_CHAINS, N_TRANSITIONS, BURN_IN = (20, 64, 12, 4) if SMOKE else (800, 2048, 300, 100)
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
device_name = torch.cuda.get_device_name(0) if device.type == "cuda" else "cpu"

torch.manual_seed(0)
centres = torch.tensor([[-1.75, 0.0], [1.75, 0.0]], device=device)


def train(data):
    energy = MLPEnergy(2, 64, device=device)
    trainer = LangevinDynamics(model=energy, step_size=0.05, noise_scale=1.0, device=device)
    pcd = ContrastiveDivergence(model=energy, sampler=trainer, k_steps=10, persistent=True, buffer_size=4096, energy_reg_weight=0.1,
                                device=device)
    opt = torch.optim.Adam(energy.parameters(), lr=1e-3)
    for step in range(TRAIN_STEPS):
        batch = data[torch.randint(len(data), (256,), device=device)]
        loss, _ = pcd(batch)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return energy, loss.item()


def confining():
    """A unimodal MLPEnergy(2, 64): every outer weight is positive, so the energy grows in every direction."""
    energy = MLPEnergy(2, 64, device=device)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        d = torch.randn(64, 2, generator=g)
        energy.net[0].weight.copy_(2.0 * d / d.norm(dim=1, keepdim=True))
        energy.net[0].bias.copy_(0.3 * torch.randn(64, generator=g))
        energy.net[2].weight.copy_(2.0 * torch.rand(64, 64, generator=g) / 64)
        energy.net[2].bias.copy_(0.1 * torch.randn(64, generator=g))
        energy.net[4].weight.copy_(8.0 * torch.rand(1, 64, generator=g) / 64)
        energy.net[4].bias.zero_()
    return energy


def diagnose(energy, start):
    sampler = GeneralizedHMC(energy, step_size=0.3, n_leapfrog_steps=5, friction=1.0, device=device)
    sampler.fused_mlp = sampler.fused_mlp_moments = True  # one launch per call on a CUDA device; the eager route elsewhere
    _, moments = sampler.sample_moments(x=start, n_steps=N_TRANSITIONS, burn_in=BURN_IN, energy=True)
    return sampler, moments


fmt = lambda t, d=3: [round(v, d) for v in t.tolist()]  # noqa: E731
print(f"device={device} ({device_name})  {N_CHAINS} chains, {N_TRANSITIONS} transitions ({BURN_IN} burnt) of generalized HMC, L = 5")

two_modes, loss = train(centres[torch.randint(2, (4000,), device=device)] + 0.3 * torch.randn(4000, 2, device=device))
start = centres[torch.arange(N_CHAINS, device=device) % 2] + 0.3 * torch.randn(N_CHAINS, 2, device=device)  # half in each blob
sampler, stuck = diagnose(two_modes, start)
print(f"two-mode network (final loss {loss:+.3f}), chains started half in each mode:  split R-hat = {fmt(stuck.rhat)}, "
      f"ESS = {fmt(stuck.ess, 0)} of {2 * N_CHAINS * stuck.half_len} counted states, energy R-hat = {float(stuck.energy_rhat):.3f}, "
      f"acceptance = {float(stuck.acceptance_rate.mean()):.3f}")

start = torch.randn(N_CHAINS, 2, device=device)
_, mixed = diagnose(confining(), start)
print(f"unimodal network, chains started from N(0, I):                             split R-hat = {fmt(mixed.rhat)}, "
      f"ESS = {fmt(mixed.ess, 0)}, energy R-hat = {float(mixed.energy_rhat):.3f}, acceptance = {float(mixed.acceptance_rate.mean()):.3f}")
print("A split R-hat well above 1 in the first coordinate says the chains of the two-mode run have not met: pooled moments of that "
      "run describe the starts, not the model.")
print("route", sampler._route(start)[0], "+ fused_mlp_moments" if sampler._route(start)[0] == "fused_mlp" else "")
