"""UnderdampedLangevin.sample on an MLP3Energy at hidden width 64: the one-launch BAOAB kernel against the eager route on the same
network, and against LangevinDynamics.sample on the same rows.

65 536 chains x 20 steps at dim 2, 32, 64 and 128.  "fused" is the sampler with the opt-in ``fused_mlp = True`` (one launch of
ebm_kinetic_chain_mlp3_f32: 21 evaluations); "eager" is the same sampler without the opt-in (21 launches of the energy's
one-launch gradient, ebm_energy_grad_mlp3_f32, and the torch element-wise updates between them); "langevin" is
LangevinDynamics.sample (one launch of ebm_langevin_chain_mlp3_f32: 20 evaluations).  The three alternate in one process: 2 warm-up
and 10 timed calls each, every call closed by a device synchronise; medians and min - max in milliseconds.  One JSON line per
shape is appended to profiles/mlp3_kinetic_bench.jsonl.

    python scripts/bench_mlp3_kinetic.py [--chains 65536] [--steps 20] [--out profiles/mlp3_kinetic_bench.jsonl]
"""

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torchebm_amd as ta  # noqa: E402
from torchebm_amd import _lib  # noqa: E402

DIMS = [2, 32, 64, 128]
HIDDEN = 64
ENTRY, GRADIENT, LANGEVIN = "ebm_kinetic_chain_mlp3_f32", "ebm_energy_grad_mlp3_f32", "ebm_langevin_chain_mlp3_f32"


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp3_kinetic_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp3_kinetic.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    for dim in DIMS:
        torch.manual_seed(HIDDEN + dim)
        model = ta.MLP3Energy(dim, HIDDEN, device=dev)
        model.KINETIC_MAX_DIM = {HIDDEN: 128}  # the kernel at every width, whatever the class default makes of these figures
        x0 = torch.randn(args.chains, dim, device=dev)
        runs = {
            "fused": ta.UnderdampedLangevin(model, step_size=0.05, device=dev),
            "eager": ta.UnderdampedLangevin(model, step_size=0.05, device=dev),
            "langevin": ta.LangevinDynamics(model, step_size=0.01, device=dev),
        }
        runs["fused"].fused_mlp = True
        assert runs["fused"]._route(x0)[0] == "fused_mlp3" and runs["eager"]._route(x0)[0] == "eager", dim
        times = {name: [] for name in runs}
        before = {e: _lib.call_counts[e] for e in (ENTRY, GRADIENT, LANGEVIN)}
        n_calls = args.warmup + args.calls
        for it in range(n_calls):
            for name, sampler in runs.items():  # alternating, in one process
                ms = _timed(lambda: sampler.sample(x=x0, n_steps=args.steps))
                if it >= args.warmup:
                    times[name].append(ms)
        # each route ran what its name says: one kernel launch per call, k + 1 gradient launches per call, one chain launch per call
        assert _lib.call_counts[ENTRY] == before[ENTRY] + n_calls
        assert _lib.call_counts[GRADIENT] == before[GRADIENT] + n_calls * (args.steps + 1)
        assert _lib.call_counts[LANGEVIN] == before[LANGEVIN] + n_calls
        rec = {"bench": "mlp3_kinetic", "hidden": HIDDEN, "dim": dim, "chains": args.chains, "steps": args.steps,
               "eager_gradient": GRADIENT, **{name: _stats(ms) for name, ms in times.items()}}
        spread = max(rec["fused"]["max_ms"] - rec["fused"]["min_ms"], rec["eager"]["max_ms"] - rec["eager"]["min_ms"])
        rec["fused_faster"] = rec["eager"]["median_ms"] - rec["fused"]["median_ms"] > spread
        rec["eager_over_fused"] = rec["eager"]["median_ms"] / rec["fused"]["median_ms"]
        rec["fused_over_langevin"] = rec["fused"]["median_ms"] / rec["langevin"]["median_ms"]
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
