"""LangevinDynamics.sample on an MLP3Energy: the one-launch chain kernel against the per-step route on the same network.

65 536 chains x 20 steps at (hidden, dim) = (64, 2), (64, 32), (128, 2), (128, 32).  The per-step route (autograd's gradient --
or, with --hip-step-gradient, the one-launch evaluation -- plus one update kernel per step, replayed from a HIP graph) is what
the sampler runs for this network without the chain kernel.  The two alternate in one process: 2 warm-up and 10 timed calls each,
every call bracketed by a device synchronise; medians and min - max in milliseconds.  For orientation the two-hidden-layer
MLPEnergy call at the same shape is timed beside them.  One JSON line per shape is appended to profiles/mlp3_bench.jsonl.

    python scripts/bench_mlp3.py [--chains 65536] [--steps 20] [--out profiles/mlp3_bench.jsonl]
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

SHAPES = [(64, 2), (64, 32), (128, 2), (128, 32)]


class _StepRoute(ta.MLP3Energy):
    """The same network with no fused spec of its own: LangevinDynamics takes the per-step route.  ``autograd`` (the default)
    leaves its gradient to autograd, the route this network had without the kernels; otherwise it is the one-launch evaluation."""

    autograd = True

    def fused_spec(self):
        return None

    def _hip_gradient(self, x, model_kwargs):
        if self.autograd or model_kwargs:
            return None
        grad = torch.empty_like(x)
        spec = ta.MLP3Energy.fused_spec(self.twin)
        _lib.call("ebm_energy_grad_mlp3_f32", spec.to_c(), x.data_ptr(), x.shape[0], x.shape[1], None, grad.data_ptr(),
                  _lib.stream_handle(x.device))
        return grad


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
    ap.add_argument("--hip-step-gradient", action="store_true", help="the per-step route's gradient by the one-launch evaluation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp3_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp3.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    for hidden, dim in SHAPES:
        torch.manual_seed(hidden + dim)
        fused = ta.MLP3Energy(dim, hidden, device=dev)
        assert fused.fused_spec() is not None, (hidden, dim)
        step = _StepRoute(dim, hidden, device=dev)
        step.net, step.twin, step.autograd = fused.net, fused, not args.hip_step_gradient
        two = ta.MLPEnergy(dim, hidden, device=dev)
        x0 = torch.randn(args.chains, dim, device=dev)
        runs = {
            "fused": ta.LangevinDynamics(fused, step_size=0.01, device=dev),
            "step": ta.LangevinDynamics(step, step_size=0.01, device=dev),
            "two_layer": ta.LangevinDynamics(two, step_size=0.01, device=dev),
        }
        runs["step"].capture_graph = True  # always the replayed graph, whatever the capture checks make of the wrapper class
        times = {name: [] for name in runs}
        for it in range(args.warmup + args.calls):
            for name, sampler in runs.items():  # alternating, in one process
                ms = _timed(lambda: sampler.sample(x=x0, n_steps=args.steps))
                if it >= args.warmup:
                    times[name].append(ms)
        rec = {"bench": "mlp3_langevin", "hidden": hidden, "dim": dim, "chains": args.chains, "steps": args.steps,
               "step_gradient": "ebm_energy_grad_mlp3_f32" if args.hip_step_gradient else "autograd",
               **{name: _stats(ms) for name, ms in times.items()}}
        spread = max(rec["fused"]["max_ms"] - rec["fused"]["min_ms"], rec["step"]["max_ms"] - rec["step"]["min_ms"])
        rec["fused_faster"] = rec["step"]["median_ms"] - rec["fused"]["median_ms"] > spread
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
