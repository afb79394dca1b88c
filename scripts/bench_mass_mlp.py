"""Cost and payoff of a mass on the fused MLP walks: one massed sample() call under fused_mlp + fused_mlp_mass -- ONE launch of
ebm_kinetic_mlp_chain_mass_f32 / ebm_ghmc_mlp_chain_mass_f32 -- against the unit-mass fused_mlp call of the same sampler and
against the massed eager call (what a massed sampler on an MLPEnergy gets without the second opt-in), alternating in one process.

2^16 chains x 32 dims on MLPEnergy(32, 128) and 65 536 x 2 on MLPEnergy(2, 128); UnderdampedLangevin with k = 20 steps,
GeneralizedHMC with 10 transitions of L = 4; a diagonal mass exp(U(-log 2, log 4)) and, beside it, the scalar mass 0.5.  An event
pair around every call and (_lib.timed_events) around every launch of the one-launch routes; 2 warm-up and 10 timed calls each.
One JSON line per shape and sampler is appended to profiles/mass_mlp_bench.jsonl.  No time is a pass/fail bar; the figures to
read are two ratios: the massed launch to the unit-mass launch of the same commit, and the eager massed call to the fused massed
call, which has to exceed 1 by more than the larger min - max spread (docs/design/mass_mlp.md)."""

import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torchebm_amd as ta  # noqa: E402
from torchebm_amd import _lib  # noqa: E402

N, HIDDEN, WARMUP, TIMED = 1 << 16, 128, 2, 10
K_BAOAB, H = 20, 0.2
N_MH, L, EPS = 10, 4, 0.3
GAMMA, TEMP = 1.5, 0.8
ENTRIES = {"baoab": ("ebm_kinetic_mlp_chain_mass_f32", "ebm_kinetic_mlp_chain_f32"),
           "ghmc": ("ebm_ghmc_mlp_chain_mass_f32", "ebm_ghmc_mlp_chain_f32")}


def once(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def summary(times):
    return {"median": round(statistics.median(times), 4), "min": round(min(times), 4), "max": round(max(times), 4)}


def spread(s):
    """(max - min) / median of a summary."""
    return (s["max"] - s["min"]) / s["median"]


def main():
    assert torch.cuda.is_available(), "bench_mass_mlp.py needs a GPU"
    dev = torch.device("cuda")
    out = os.path.join(ROOT, "profiles", "mass_mlp_bench.jsonl")
    for dim in (32, 2):
        torch.manual_seed(10 + dim)
        model = ta.MLPEnergy(dim, HIDDEN, device=dev)
        mass = torch.exp(-math.log(2.0) + math.log(8.0) * torch.rand(dim, generator=torch.Generator().manual_seed(0))).to(dev)
        scale = math.sqrt(float(mass.min()))  # the massed calls step by sqrt(min m)
        makers = {
            "baoab": (lambda m, f: ta.UnderdampedLangevin(model, step_size=H * f, friction=GAMMA, temperature=TEMP, device=dev, mass=m), K_BAOAB),
            "ghmc": (lambda m, f: ta.GeneralizedHMC(model, step_size=EPS * f, n_leapfrog_steps=L, friction=GAMMA, temperature=TEMP,
                                                    device=dev, mass=m), N_MH),
        }
        for label, (make, steps) in makers.items():
            massed_entry, unit_entry = ENTRIES[label]
            unit, diag, scalar, eager = make(None, 1.0), make(mass, scale), make(0.5, math.sqrt(0.5)), make(mass, scale)
            unit.fused_mlp = True
            for s in (diag, scalar):
                s.fused_mlp = s.fused_mlp_mass = True
            eager.fused_mlp = True  # the parent commit's route for a massed MLP sampler
            x0 = torch.randn(N, dim, device=dev)
            assert unit._route(x0)[0] == "fused_mlp" and diag._route(x0)[0] == scalar._route(x0)[0] == "fused_mlp_mass"
            assert eager._route(x0)[0] == "eager"
            g = torch.Generator(device=dev).manual_seed(0)
            calls = {"diag": lambda: diag.sample(x=x0, n_steps=steps, generator=g),
                     "scalar": lambda: scalar.sample(x=x0, n_steps=steps, generator=g),
                     "unit": lambda: unit.sample(x=x0, n_steps=steps, generator=g),
                     "eager": lambda: eager.sample(x=x0, n_steps=steps, generator=g)}
            times = {key: [] for key in calls}
            for i in range(WARMUP + TIMED):
                if i == WARMUP:
                    torch.cuda.synchronize()
                    _lib.timed_events[massed_entry], _lib.timed_events[unit_entry] = [], []
                for key, fn in calls.items():  # alternating in one process
                    t = once(fn)
                    if i >= WARMUP:
                        times[key].append(t)
            torch.cuda.synchronize()
            massed_launches = [a.elapsed_time(b) for a, b in _lib.timed_events.pop(massed_entry)]  # diag, scalar, diag, ...
            unit_launches = [a.elapsed_time(b) for a, b in _lib.timed_events.pop(unit_entry)]
            assert len(massed_launches) == 2 * TIMED and len(unit_launches) == TIMED
            row = {"case": f"MLPEnergy({dim}, {HIDDEN})", "sampler": label, "n": N, "dim": dim, "steps": steps,
                   "n_leapfrog": L if label == "ghmc" else None, "warmup": WARMUP, "timed": TIMED, "unit": "ms",
                   "device": torch.cuda.get_device_name(0),
                   "diag_call": summary(times["diag"]), "scalar_call": summary(times["scalar"]), "unit_call": summary(times["unit"]),
                   "eager_call": summary(times["eager"]),
                   "diag_launch": summary(massed_launches[0::2]), "scalar_launch": summary(massed_launches[1::2]),
                   "unit_launch": summary(unit_launches)}
            row["ratio_diag_launch_to_unit_launch"] = round(row["diag_launch"]["median"] / row["unit_launch"]["median"], 3)
            row["ratio_scalar_launch_to_unit_launch"] = round(row["scalar_launch"]["median"] / row["unit_launch"]["median"], 3)
            row["ratio_eager_call_to_diag_call"] = round(row["eager_call"]["median"] / row["diag_call"]["median"], 2)
            row["larger_spread"] = round(max(spread(row["eager_call"]), spread(row["diag_call"])), 3)
            row["pass"] = row["ratio_eager_call_to_diag_call"] > 1.0 + row["larger_spread"]
            print(json.dumps(row))
            with open(out, "a") as f:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
