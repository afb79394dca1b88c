"""Cost of a mass: one massed sample() call -- ONE launch of ebm_kinetic_chain_mass_f32 / ebm_ghmc_chain_mass_f32 -- against the
unit-mass call of the same sampler on the same rows in the same process.

2^16 chains x 32 dims on the double well and on ring_mixture(8, 32); UnderdampedLangevin with k = 200 steps, GeneralizedHMC with
n_mh = 50 and L = 4; a diagonal mass exp(U(-log 2, log 4)) and, beside it, the scalar mass 0.5 (no division per coordinate in the
kinetic energy).  Event pairs around the call, 2 warm-up and 10 timed calls per sampler, the calls alternating; one JSON line per
energy and sampler is appended to profiles/mass_bench.jsonl.  No time is a pass/fail bar: the figure to read is the ratio to
the unit-mass call of the same commit (from the code: one division and one product per coordinate in front of the loop, two or
three more slices of registers per lane -- which is what generalized HMC pays for: docs/design/mass.md)."""

import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torchebm_amd as ta  # noqa: E402

N, DIM, WARMUP, TIMED = 1 << 16, 32, 2, 10
K_BAOAB, H = 200, 0.05
N_MH, L, EPS = 50, 4, 0.05


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
    assert torch.cuda.is_available(), "bench_mass.py needs a GPU"
    dev = torch.device("cuda")
    energies = {"double_well": ta.DoubleWellModel(device=dev), "ring_mixture_8": ta.core.ring_mixture(8, DIM, device=dev)}
    mass = torch.exp(-math.log(2.0) + math.log(8.0) * torch.rand(DIM, generator=torch.Generator().manual_seed(0))).to(dev)
    scale = math.sqrt(float(mass.min()))  # the massed call steps by sqrt(min m): h^2 E'' / m stays what the unit-mass call runs at
    out = os.path.join(ROOT, "profiles", "mass_bench.jsonl")
    for name, model in energies.items():
        samplers = {
            "baoab": (lambda m, f: ta.UnderdampedLangevin(model, step_size=H * f, friction=1.0, temperature=1.0, device=dev, mass=m), K_BAOAB),
            "ghmc": (lambda m, f: ta.GeneralizedHMC(model, step_size=EPS * f, n_leapfrog_steps=L, friction=1.0, temperature=1.0, device=dev,
                                                    mass=m), N_MH),
        }
        for label, (make, steps) in samplers.items():
            unit, massed, scalar = make(None, 1.0), make(mass, scale), make(0.5, math.sqrt(0.5))
            x0 = torch.randn(N, DIM, device=dev)
            assert unit._route(x0)[0] == "fused" and massed._route(x0)[0] == "fused_mass"
            g = torch.Generator(device=dev).manual_seed(0)
            calls = {"mass": lambda: massed.sample(x=x0, n_steps=steps, generator=g),
                     "scalar": lambda: scalar.sample(x=x0, n_steps=steps, generator=g),
                     "unit": lambda: unit.sample(x=x0, n_steps=steps, generator=g)}
            times = {key: [] for key in calls}
            for i in range(WARMUP + TIMED):
                for key, fn in calls.items():  # alternating in one process
                    t = once(fn)
                    if i >= WARMUP:
                        times[key].append(t)
            row = {"case": name, "sampler": label, "n": N, "dim": DIM, "steps": steps, "n_leapfrog": L if label == "ghmc" else None,
                   "warmup": WARMUP, "timed": TIMED, "unit": "ms", "device": torch.cuda.get_device_name(0), "mass": summary(times["mass"]),
                   "scalar_mass": summary(times["scalar"]), "unit_mass": summary(times["unit"])}
            row["ratio_mass_to_unit"] = round(row["mass"]["median"] / row["unit_mass"]["median"], 3)
            row["ratio_scalar_to_unit"] = round(row["scalar_mass"]["median"] / row["unit_mass"]["median"], 3)
            print(json.dumps(row))
            with open(out, "a") as f:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
