"""LangevinDynamics.sample on an MLP3Energy at hidden width 128: the streamed bf16 chain kernel against the route the same network
has without it.

65 536 chains x 20 steps.  At dim 2 and 32 the other route is the exact-f32 chain kernel (``streamed_bf16 = False``, the
default there); at dim 33, 64 and 128 it is the per-step route with autograd's gradient, replayed from a HIP graph, which is all
these widths had.  The two alternate in one process: 2 warm-up and 10 timed calls each, every call closed by a device
synchronise; medians and min - max in milliseconds.  One JSON line per shape is appended to profiles/mlp3_stream_bench.jsonl.

    python scripts/bench_mlp3_stream.py [--chains 65536] [--steps 20] [--out profiles/mlp3_stream_bench.jsonl]
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

HIDDEN = 128
DIMS = [2, 32, 33, 64, 128]


class _StepRoute(ta.MLP3Energy):
    """The same network with no fused spec and autograd's gradient: LangevinDynamics takes the per-step route."""

    def fused_spec(self):
        return None

    def _hip_gradient(self, x, model_kwargs):
        return None


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp3_stream_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp3_stream.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    for dim in DIMS:
        torch.manual_seed(HIDDEN + dim)
        streamed = ta.MLP3Energy(dim, HIDDEN, device=dev)
        streamed.streamed_bf16 = True
        assert streamed.fused_spec().aux is not None, dim
        if dim <= ta.MLP3Energy.FUSED_MAX_DIM[HIDDEN]:
            other_name, other = "exact_f32", ta.MLP3Energy(dim, HIDDEN, device=dev)
            assert other.fused_spec().aux is None, dim
        else:
            other_name, other = "step_autograd", _StepRoute(dim, HIDDEN, device=dev)
        other.net = streamed.net
        x0 = torch.randn(args.chains, dim, device=dev)
        runs = {"streamed": ta.LangevinDynamics(streamed, step_size=0.01, device=dev),
                other_name: ta.LangevinDynamics(other, step_size=0.01, device=dev)}
        if other_name == "step_autograd":
            runs[other_name].capture_graph = True  # always the replayed graph, whatever the capture checks make of the wrapper class
        times = {name: [] for name in runs}
        for it in range(args.warmup + args.calls):
            for name, sampler in runs.items():  # alternating, in one process
                ms = _timed(lambda: sampler.sample(x=x0, n_steps=args.steps))
                if it >= args.warmup:
                    times[name].append(ms)
        rec = {"bench": "mlp3_stream_langevin", "hidden": HIDDEN, "dim": dim, "chains": args.chains, "steps": args.steps,
               "other": other_name, **{name: _stats(ms) for name, ms in times.items()}}
        spread = max(rec[name]["max_ms"] - rec[name]["min_ms"] for name in runs)
        rec["ratio"] = rec[other_name]["median_ms"] / rec["streamed"]["median_ms"]
        rec["streamed_faster"] = rec[other_name]["median_ms"] - rec["streamed"]["median_ms"] > spread
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
