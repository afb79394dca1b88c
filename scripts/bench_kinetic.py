"""Cost of underdamped Langevin (BAOAB): one UnderdampedLangevin.sample() call -- ONE launch of ebm_kinetic_chain_f32 -- against
LangevinDynamics.sample() on the same rows in the same process.

2^16 chains x 32 dims, k = 200, on the double well and on ring_mixture(8, 32).  Event pairs around the call, 2 warm-up and 10
timed calls per sampler, the two samplers alternating; one JSON line per energy is appended to profiles/kinetic_bench.jsonl.
No time is a pass/fail bar: the figure to read is the ratio to the plain Langevin call of the same commit."""

import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torchebm_amd as ta  # noqa: E402

N, DIM, K, WARMUP, TIMED = 1 << 16, 32, 200, 2, 10


def once(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def summary(times):
    return {"median": round(statistics.median(times), 4), "min": round(min(times), 4), "max": round(max(times), 4)}


def main():
    assert torch.cuda.is_available(), "bench_kinetic.py needs a GPU"
    dev = torch.device("cuda")
    energies = {"double_well": ta.DoubleWellModel(device=dev), "ring_mixture_8": ta.core.ring_mixture(8, DIM, device=dev)}
    out = os.path.join(ROOT, "profiles", "kinetic_bench.jsonl")
    for name, model in energies.items():
        # matching steps: Euler-Maruyama's eta = h^2 / 2
        kinetic = ta.UnderdampedLangevin(model, step_size=0.1, friction=1.0, temperature=1.0, device=dev)
        plain = ta.LangevinDynamics(model, step_size=0.005, device=dev)
        x0 = torch.randn(N, DIM, device=dev)
        assert kinetic._route(x0)[0] == "fused"
        g = torch.Generator(device=dev).manual_seed(0)
        calls = {"kinetic": lambda: kinetic.sample(x=x0, n_steps=K, generator=g), "langevin": lambda: plain.sample(x=x0, n_steps=K, generator=g)}
        times = {label: [] for label in calls}
        for i in range(WARMUP + TIMED):
            for label, fn in calls.items():  # alternating in one process
                t = once(fn)
                if i >= WARMUP:
                    times[label].append(t)
        row = {"case": name, "n": N, "dim": DIM, "k": K, "warmup": WARMUP, "timed": TIMED, "unit": "ms",
               "device": torch.cuda.get_device_name(0), "kinetic": summary(times["kinetic"]), "langevin": summary(times["langevin"])}
        row["ratio_kinetic_to_langevin"] = round(row["kinetic"]["median"] / row["langevin"]["median"], 3)
        print(json.dumps(row))
        with open(out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
