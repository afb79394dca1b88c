"""Cost of per-chain running moments under the two velocity-carrying samplers: one sample_moments() call against the same
steps through sample(), and against what a user had before -- sample(return_trajectory=True, thin=1) followed by torch moments
of the trajectory.

2^16 chains x 32 dims, k = 200: BAOAB and generalized HMC (L = 3) on the double well and on ring_mixture(8, 32).  The three
variants of a case run in the same process, alternating: every round times each of them once (event pairs), 2 warm-up and 10
timed rounds; one JSON line per case is appended to profiles/kinetic_moments_bench.jsonl (or to the path given as argument)."""

import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torchebm_amd as ta  # noqa: E402

N, DIM, K, WARMUP, TIMED = 1 << 16, 32, 200, 2, 10


def timed_alternating(variants):
    times = {label: [] for label, _ in variants}
    for i in range(WARMUP + TIMED):
        for label, fn in variants:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            if i >= WARMUP:
                times[label].append(start.elapsed_time(stop))
    return {label: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)} for label, t in times.items()}


def trajectory_moments(sampler, x0, g):
    traj = sampler.sample(x=x0, n_steps=K, return_trajectory=True, thin=1, generator=g)  # [n, k, dim]
    halves = traj.view(N, 2, K // 2, DIM)
    mean = halves.mean(dim=2)
    return mean, ((halves - mean.unsqueeze(2)) ** 2).sum(dim=2)


def main():
    assert torch.cuda.is_available(), "bench_kinetic_moments.py needs a GPU"
    dev = torch.device("cuda")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "kinetic_moments_bench.jsonl")
    energies = {"double_well": (ta.DoubleWellModel(device=dev), 0.05, 0.1), "ring_mixture": (ta.core.ring_mixture(8, DIM, device=dev), 0.3, 0.3)}
    cases = {}
    for name, (model, h, eps) in energies.items():
        cases["baoab_" + name] = ta.UnderdampedLangevin(model, step_size=h, device=dev)
        cases["ghmc_L3_" + name] = ta.GeneralizedHMC(model, step_size=eps, n_leapfrog_steps=3, device=dev)
    for name, s in cases.items():
        x0 = torch.randn(N, DIM, device=dev)
        g = torch.Generator(device=dev).manual_seed(0)
        row = {"case": name, "n": N, "dim": DIM, "k": K, "warmup": WARMUP, "timed": TIMED, "unit": "ms", "device": torch.cuda.get_device_name(0)}
        row.update(timed_alternating((
            ("sample_moments", lambda: s.sample_moments(x=x0, n_steps=K, generator=g)),
            ("sample", lambda: s.sample(x=x0, n_steps=K, generator=g)),
            ("trajectory_then_torch_moments", lambda: trajectory_moments(s, x0, g)),
        )))
        print(json.dumps(row), flush=True)
        with open(out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
