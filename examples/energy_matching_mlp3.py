"""Adopt the hand-written three-hidden-layer energy network of the reference's energy-matching examples and sample it.

The examples write ``Linear(2, H) - SiLU - Linear(H, H) - SiLU - Linear(H, H) - SiLU - Linear(H, 1)`` as a plain
``nn.Sequential``.  ``MLP3Energy.from_sequential`` wraps that stack without copying it -- an optimiser built on ``net`` keeps
training the same tensors -- and on a CUDA device every ``LangevinDynamics.sample`` call below is ONE kernel launch and every
``gradient`` call another.  On a CPU the same script runs the per-step route.

    python examples/energy_matching_mlp3.py [dim]

``dim`` (default 2, at least 2) is the input width: the two moons sit in the first two coordinates and the others are Gaussian noise.  At
hidden width 128 a width of 33 .. 128 (say 64) runs the streamed bf16 kernel (docs/design/mlp3_stream.md).
"""

import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torchebm_amd as ta  # noqa: E402


def main():
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    torch.manual_seed(0)
    hidden, dim = 128, int(sys.argv[1]) if len(sys.argv) > 1 else 2
    if dim < 2:
        raise SystemExit("dim must be at least 2: the two moons need two coordinates")
    net = nn.Sequential(
        nn.Linear(dim, hidden), nn.SiLU(), nn.Linear(hidden, hidden), nn.SiLU(), nn.Linear(hidden, hidden), nn.SiLU(), nn.Linear(hidden, 1)
    ).to(device)
    energy = ta.MLP3Energy.from_sequential(net)
    assert energy.net is net

    # a few steps of a contrastive fit to two moons, negatives drawn by Langevin dynamics on the current energy
    data = ta.datasets.TwoMoonsDataset(n_samples=2048, noise=0.05, seed=0).get_data().to(device)
    data = torch.cat([data, 0.1 * torch.randn(data.shape[0], dim - 2, device=device)], dim=1)
    sampler = ta.LangevinDynamics(energy, step_size=0.01, noise_scale=0.1, device=device)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    for it in range(20):
        negatives = sampler.sample(x=torch.randn_like(data), n_steps=20)
        loss = energy(data).mean() - energy(negatives.detach()).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    samples = sampler.sample(x=torch.randn(4096, dim, device=device), n_steps=100)
    grad = energy.gradient(samples)
    print(f"device {device.type}: loss {loss.item():+.4f}, sample std {samples.std(0)[:2].tolist()}, mean |grad| {grad.abs().mean().item():.4f}")


if __name__ == "__main__":
    main()
