#!/usr/bin/env python3
"""sample() on the fused route against the step route for the three landscape energies (Rosenbrock, Ackley, Rastrigin):
one JSON line per (energy, sampler, shape, route).  The step route is what these models took before they had a fused
spec -- autograd gradient plus one update kernel per step -- and is reached here the way a user reaches it: a subclass
that overrides ``forward`` is not fused.  Both routes are timed alternately in one process: device events around
windows of three whole sample() calls each (start states copied outside the window), five windows per route, after two
warm-up calls of each; median and minimum of the windows are reported.  Run on the GPU:

    python scripts/bench_landscapes.py [--quick] [--out profiles/landscapes_bench.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torchebm_amd as ta  # noqa: E402
from torchebm_amd import _lib  # noqa: E402
from torchebm_amd.core import AckleyModel, RastriginModel, RosenbrockModel  # noqa: E402


def unfused(cls):
    class Step(cls):
        def forward(self, x):  # the same function: only the fused descriptor goes
            return super().forward(x)

    Step.__name__ = cls.__name__ + "StepRoute"
    return Step


def timed(fn, starts):
    """milliseconds per call of fn(x) over the prepared start states (their copies are made outside the timed window)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for x in starts:
        fn(x)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / len(starts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one round, the small shape only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_landscapes.py needs a GPU"
    dev = torch.device("cuda")
    shapes = [(1024, 128)] if args.quick else [(1 << 18, 32), (1024, 128)]
    rounds, reps = (1, 2) if args.quick else (5, 3)  # both routes: `reps` calls per window, `rounds` windows, alternating
    lines = []
    for cls, step in ((RosenbrockModel, 1e-4), (AckleyModel, 1e-2), (RastriginModel, 1e-3)):
        models = {"fused": cls(device=dev), "step": unfused(cls)(device=dev)}
        assert models["fused"].fused_spec() is not None and models["step"].fused_spec() is None
        for n, dim in shapes:
            x0 = (torch.rand(n, dim, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2 - 1)
            for sampler in ("langevin", "hmc"):
                runs = {}
                for route, m in models.items():
                    if sampler == "langevin":
                        s = ta.LangevinDynamics(m, step_size=step, device=dev)
                        runs[route] = lambda x, s=s: s.sample(x=x, n_steps=100)
                    else:
                        s = ta.HamiltonianMonteCarlo(m, step_size=step, n_leapfrog_steps=10, device=dev)
                        runs[route] = lambda x, s=s: s.sample(x=x, n_steps=10)
                for fn in runs.values():  # warm-up: code objects, graph capture of the step route
                    fn(x0.clone())
                    fn(x0.clone())
                torch.cuda.synchronize()
                before = dict(_lib.call_counts)
                ms = {r: [] for r in runs}
                for _ in range(rounds):
                    for r, fn in runs.items():
                        ms[r].append(timed(fn, [x0.clone() for _ in range(reps)]))
                calls = {k: v - before.get(k, 0) for k, v in _lib.call_counts.items() if v != before.get(k, 0)}
                work = n * 100  # chain steps (Langevin) or leapfrog steps (HMC: 10 transitions of 10) per call
                for r in runs:
                    t = sorted(ms[r])
                    lines.append({"energy": cls.__name__, "sampler": sampler, "n": n, "dim": dim, "route": r,
                                  "ms_median": round(t[len(t) // 2], 4), "ms_min": round(t[0], 4),
                                  "chain_steps_per_s": work / (t[len(t) // 2] * 1e-3), "entry_calls": calls if r == "step" else None})
                    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
