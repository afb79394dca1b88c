"""Cost of the step-size adaptation: one GeneralizedHMC.adapt_step_size() call -- ONE launch of ebm_ghmc_adapt_chain_f32 --
against GeneralizedHMC.sample() with the same leapfrog count and transition count on the same rows in the same process.

2^16 chains x 32 dims, 50 transitions, L = 4, on the double well and on ring_mixture(8, 32).  Event pairs around the call, 2
warm-up and 10 timed calls per method, the two alternating; one JSON line per energy is appended to
profiles/ghmc_adapt_bench.jsonl.  adapt_step_size runs with apply=False, so neither call reads anything back.  No time is a
pass/fail bar: the figure to read is the ratio to the sample() call of the same commit (from the code: the same trajectory plus
two transcendental calls per chain and transition for the refresh constants, one more for the controller, and three floats per
chain of traffic)."""

import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torchebm_amd as ta  # noqa: E402
from torchebm_amd.samplers.adapt import adapt_route  # noqa: E402

N, DIM, N_MH, L, EPS, WARMUP, TIMED = 1 << 16, 32, 50, 4, 0.05, 2, 10


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
    assert torch.cuda.is_available(), "bench_ghmc_adapt.py needs a GPU"
    dev = torch.device("cuda")
    energies = {"double_well": ta.DoubleWellModel(device=dev), "ring_mixture_8": ta.core.ring_mixture(8, DIM, device=dev)}
    out = os.path.join(ROOT, "profiles", "ghmc_adapt_bench.jsonl")
    for name, model in energies.items():
        ghmc = ta.GeneralizedHMC(model, step_size=EPS, n_leapfrog_steps=L, friction=1.0, temperature=1.0, device=dev)
        x0 = torch.randn(N, DIM, device=dev)
        assert ghmc._route(x0)[0] == "fused" and adapt_route(ghmc, x0, 1.0)[0] == "fused"
        g = torch.Generator(device=dev).manual_seed(0)
        calls = {"adapt": lambda: ghmc.adapt_step_size(x=x0, n_steps=N_MH, generator=g, apply=False),
                 "sample": lambda: ghmc.sample(x=x0, n_steps=N_MH, generator=g)}
        times = {label: [] for label in calls}
        for i in range(WARMUP + TIMED):
            for label, fn in calls.items():  # alternating in one process
                t = once(fn)
                if i >= WARMUP:
                    times[label].append(t)
        row = {"case": name, "n": N, "dim": DIM, "n_mh": N_MH, "n_leapfrog": L, "eps": EPS, "warmup": WARMUP, "timed": TIMED, "unit": "ms",
               "device": torch.cuda.get_device_name(0), "adapt": summary(times["adapt"]), "sample": summary(times["sample"])}
        row["ratio_adapt_to_sample"] = round(row["adapt"]["median"] / row["sample"]["median"], 3)
        print(json.dumps(row))
        with open(out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
