"""Let the sampler find its own step size: dual-averaging adaptation, then a production run at the result.

Every chain of a GeneralizedHMC sampler on ring_mixture(8, 32) starts at a step size far too small (0.01: every proposal is
accepted and nothing moves) and adapts its OWN step size towards an acceptance of 0.8 (Hoffman & Gelman 2014, section 3.2: the
warm-up Stan and NumPyro run).  The sampler's step size becomes the median of the chains' results, and the production run
samples at it.  The production acceptance comes out somewhat ABOVE the target -- 0.85 to 0.87 for a target of 0.8 -- because
the step size a chain ends on is the averaged iterate, which is smaller than the iterates the adaptation ran at.

    python examples/adapt_step_size.py

On a CUDA device the adaptation is one fused launch, and so is the production run."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torchebm_amd as ta  # noqa: E402
from torchebm_amd.samplers import GeneralizedHMC  # noqa: E402

SMOKE = os.environ.get("TORCHEBM_SMOKE") == "1"
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
TARGET, EPS0, L = 0.8, 0.01, 4
N, WARMUP, STEPS = (256, 100, 50) if SMOKE else (4096, 200, 200)

energy = ta.core.ring_mixture(8, 32, device=device)
sampler = GeneralizedHMC(energy, step_size=EPS0, n_leapfrog_steps=L, friction=1.0, device=device)
start = torch.randn(N, 32, generator=torch.Generator().manual_seed(0)).to(device)
g = torch.Generator(device=device).manual_seed(1)

print(f"device: {device}  chains: {N} x 32  warm-up: {WARMUP} transitions from eps = {EPS0}, L = {L}")
result = sampler.adapt_step_size(x=start, n_steps=WARMUP, target_accept=TARGET, generator=g)
logs = result.step_sizes.log()
print(f"target acceptance:              {TARGET:.3f}")
print(f"acceptance while adapting:      {result.acceptance.mean().item():.3f}   (the mean over chains and warm-up transitions)")
print(f"adapted step size:              {float(result.step_size):.4f}   (median over chains; std of log eps over chains {logs.std().item():.3f})")
assert sampler.get_scheduled_value("step_size") == float(result.step_size)

x, diag = sampler.sample(x=result.x, n_steps=STEPS, velocity=result.velocity, return_diagnostics=True, generator=g)
print(f"acceptance of the production run: {diag['acceptance_rate'].mean().item():.3f}   ({STEPS} transitions at the adapted step size)")
