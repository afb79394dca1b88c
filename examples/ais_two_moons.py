"""How good is a trained energy-based model?  Persistent contrastive divergence on two-moons for a few hundred steps, then the
mean log-likelihood of held-out data, -E(x) - log Z, with log Z from annealed importance sampling.

The energy is the packaged 2-128-128-1 SiLU `MLPEnergy`.  With `fused_mlp = True` the whole estimate -- the start draw, every
weight update and every Metropolis-corrected HMC transition on the tempered path, the network evaluated on the matrix cores --
is ONE HIP kernel launch on a CUDA device; without the opt-in (or on the CPU) the same algorithm runs in torch ops.  Nothing but
training makes a learned energy normalisable: the estimate's standard error and the effective sample size of its weights say
whether the walk covered it, so read them before the likelihood."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

from torchebm_amd.core import MLPEnergy
from torchebm_amd.losses import ContrastiveDivergence
from torchebm_amd.samplers import AnnealedImportanceSampling, LangevinDynamics
from torchebm_amd.utils.synthetic import two_moons

SMOKE = os.getenv("TORCHEBM_SMOKE") == "1"
N_STEPS, N_CHAINS, T = (20, 256, 16) if SMOKE else (400, 4096, 256)
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")

torch.manual_seed(0)
train = two_moons(n_samples=3000, noise=0.05, seed=0, device=device)
held_out = two_moons(n_samples=1000, noise=0.05, seed=1, device=device)
energy = MLPEnergy(2, device=device)
sampler = LangevinDynamics(model=energy, step_size=0.1, noise_scale=1.0, device=device)
pcd = ContrastiveDivergence(model=energy, sampler=sampler, k_steps=10, persistent=True, buffer_size=8192, device=device)
opt = torch.optim.Adam(energy.parameters(), lr=1e-3)


def held_out_log_likelihood(tag):
    ais = AnnealedImportanceSampling(energy, n_temperatures=T, schedule="sigmoid", step_size=0.25, n_leapfrog_steps=5,
                                     base_std=1.5, device=device)
    ais.fused_mlp = True  # one ebm_ais_mlp_chain_f32 launch on a CUDA device; the eager route elsewhere
    r = ais.run(N_CHAINS, 2)
    ll = ais.log_likelihood(held_out, r).mean().item()
    print(f"{tag}: route {ais._route(2)[0]}, log Z = {r.log_z:.4f} +- {r.log_z_stderr:.4f}, ESS {r.ess:.0f} of {N_CHAINS}, "
          f"acceptance {r.acceptance_rate.min().item():.2f} - {r.acceptance_rate.max().item():.2f}, "
          f"held-out mean log-likelihood {ll:+.4f}")
    return ll


for step in range(N_STEPS):
    batch = train[torch.randint(len(train), (256,), device=device)]
    loss, _ = pcd(batch)
    opt.zero_grad()
    loss.backward()
    opt.step()
    if step % 100 == 0 or step == N_STEPS - 1:
        print(f"step {step:4d}  loss {loss.item():+.3f}")
held_out_log_likelihood(f"after {N_STEPS} PCD steps")
print("done on", device)
