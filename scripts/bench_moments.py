"""Cost of per-chain running moments: one sample_moments() call against the same steps through sample(), and against what a
user had before -- sample(return_trajectory=True, thin=1) followed by torch moments of the trajectory.

2^16 chains x 32 dims, k = 200: Langevin on the double well, HMC with L = 5 on ring_mixture(8, 32).  Event pairs, 2 warm-up and
10 timed calls per variant; one JSON line per case is appended to profiles/moments_bench.jsonl."""

import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torchebm_amd as ta  # noqa: E402

N, DIM, K, WARMUP, TIMED = 1 << 16, 32, 200, 2, 10


def timed(fn):
    times = []
    for i in range(WARMUP + TIMED):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        if i >= WARMUP:
            times.append(start.elapsed_time(stop))
    return statistics.median(times), min(times), max(times)


def trajectory_moments(sampler, x0, g):
    traj = sampler.sample(x=x0, n_steps=K, return_trajectory=True, thin=1, generator=g)  # [n, k, dim]
    halves = traj.view(N, 2, K // 2, DIM)
    mean = halves.mean(dim=2)
    return mean, ((halves - mean.unsqueeze(2)) ** 2).sum(dim=2)


def main():
    assert torch.cuda.is_available(), "bench_moments.py needs a GPU"
    dev = torch.device("cuda")
    cases = {
        "langevin_double_well": ta.LangevinDynamics(ta.DoubleWellModel(device=dev), step_size=0.01, device=dev),
        "hmc_L5_ring_mixture": ta.HamiltonianMonteCarlo(ta.core.ring_mixture(8, DIM, device=dev), step_size=0.3, n_leapfrog_steps=5,
                                                        device=dev),
    }
    out = os.path.join(ROOT, "profiles", "moments_bench.jsonl")
    for name, s in cases.items():
        x0 = torch.randn(N, DIM, device=dev)
        g = torch.Generator(device=dev).manual_seed(0)
        row = {"case": name, "n": N, "dim": DIM, "k": K, "warmup": WARMUP, "timed": TIMED, "unit": "ms", "device": torch.cuda.get_device_name(0)}
        for label, fn in (
            ("sample_moments", lambda: s.sample_moments(x=x0, n_steps=K, generator=g)),
            ("sample", lambda: s.sample(x=x0, n_steps=K, generator=g)),
            ("trajectory_then_torch_moments", lambda: trajectory_moments(s, x0, g)),
        ):
            med, lo, hi = timed(fn)
            row[label] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
        print(json.dumps(row))
        with open(out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
