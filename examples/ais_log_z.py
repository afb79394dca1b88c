"""log Z of two energies by annealed importance sampling, against numbers that can be checked.

DoubleWellModel(barrier_height=2) in 4 dimensions factorises: log Z = 4 log of a one-dimensional integral, done here by
quadrature.  The eight-mode ring mixture (radius 3, sigma 0.5, 5 dimensions) is a normalised density times a known constant:
log Z = 2.5 log(2 pi 0.25).  Every estimate comes with its own standard error and the effective sample size of its weights;
with log Z in hand, -E(x) - log Z is the log-likelihood of held-out data.  On a CUDA device each estimate is one fused HIP
kernel launch."""

import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

from torchebm_amd.core import DoubleWellModel, ring_mixture
from torchebm_amd.samplers import AnnealedImportanceSampling

SMOKE = os.getenv("TORCHEBM_SMOKE") == "1"
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
device_name = torch.cuda.get_device_name(0) if device.type == "cuda" else "cpu"
n, T = (256, 16) if SMOKE else (4096, 64)
print(f"device={device} ({device_name})  {n} chains, {T} temperatures")

grid = torch.linspace(-6.0, 6.0, 200001, dtype=torch.float64)
targets = [
    ("double well, dim 4", DoubleWellModel(barrier_height=2.0, b=1.0, device=device), 4, 1.0, 0.15,
     4 * math.log(torch.trapezoid(torch.exp(-2.0 * (grid * grid - 1.0) ** 2), grid).item())),
    ("ring mixture, dim 5", ring_mixture(8, 5, radius=3.0, sigma=0.5, device=device), 5, 2.5, 0.3,
     2.5 * math.log(2 * math.pi * 0.25)),
]
for name, energy, dim, base_std, eps, truth in targets:
    ais = AnnealedImportanceSampling(energy, n_temperatures=T, schedule="linear", step_size=eps, n_leapfrog_steps=3,
                                     base_std=base_std, device=device)
    r = ais.run(n, dim)
    print(f"{name}: log Z = {r.log_z:.4f} +- {r.log_z_stderr:.4f}  (truth {truth:.4f}, {(r.log_z - truth) / r.log_z_stderr:+.1f} sigma)  "
          f"ESS {r.ess:.0f} of {n}, acceptance {r.acceptance_rate.min().item():.2f} - {r.acceptance_rate.max().item():.2f}")
    held_out = r.samples[:5]
    print("   log-likelihood of five of its own samples:", [round(v, 3) for v in ais.log_likelihood(held_out, r).tolist()])
