"""Error of the fp32 Welford recurrence of ebm_chain_moments_f32 against float64 two-pass moments of the same trajectory
(the table of docs/design/moments.md).  CPU only: the recurrence is the restatement of tests/moments_cases.py, the trajectory
the AR(1) chain of the closed-form test (HarmonicModel(k=4) under Langevin, step 0.05), as it is and shifted by three standard
deviations.  Errors are relative to the sequence's standard deviation."""

import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torchebm_amd as ta  # noqa: E402
from moments_cases import two_pass, welford  # noqa: E402

SD = math.sqrt(2 * 0.05 / 0.36)

for h in (200, 5000):
    torch.manual_seed(0)
    s = ta.LangevinDynamics(ta.HarmonicModel(k=4.0), step_size=0.05)
    x0 = SD * torch.randn(256, 4)
    traj = s.sample(x=x0, n_steps=2 * h, return_trajectory=True, generator=torch.Generator().manual_seed(1))
    for name, tr in (("mean 0", traj), ("mean 3 sd", traj + 3 * SD)):
        mean, m2 = welford(tr, h)
        mean64, m264 = two_pass(tr, h)
        sd = torch.sqrt(m264 / (h - 1))
        e_mean = ((mean.double() - mean64).abs() / sd).flatten()
        e_sd = ((torch.sqrt(m2.double() / (h - 1)) - sd).abs() / sd).flatten()
        print(f"h = {h:5d}  {name:10s}  mean: median {e_mean.median():.1e} max {e_mean.max():.1e}   "
              f"standard deviation: median {e_sd.median():.1e} max {e_sd.max():.1e}")
