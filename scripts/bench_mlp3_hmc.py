"""HamiltonianMonteCarlo.sample on an MLP3Energy at hidden width 64: the one-launch transition kernel against the per-transition
route on the same network.

65 536 chains x 10 transitions x L = 5 at dim 2, 32, 64 and 128.  The per-transition route (L + 2 evaluation launches -- the
energy's one-launch gradient, ebm_energy_grad_mlp3_f32 -- plus kick, drift and accept kernels, replayed from a HIP graph) is what
the sampler runs for this network without the kernel.  The two alternate in one process: 2 warm-up and 10 timed calls each, every
call closed by a device synchronise; medians and min - max in milliseconds.  One JSON line per shape is appended to
profiles/mlp3_hmc_bench.jsonl.

    python scripts/bench_mlp3_hmc.py [--chains 65536] [--steps 10] [--leapfrog 5] [--out profiles/mlp3_hmc_bench.jsonl]
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


class _StepRoute(ta.MLP3Energy):
    """The same network with no fused spec of its own: HamiltonianMonteCarlo takes the per-transition route, whose gradient is
    the one-launch evaluation on the twin's parameters."""

    def fused_spec(self):
        return None

    def _hip_gradient(self, x, model_kwargs):
        if model_kwargs:
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--leapfrog", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp3_hmc_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp3_hmc.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    for dim in DIMS:
        torch.manual_seed(HIDDEN + dim)
        fused = ta.MLP3Energy(dim, HIDDEN, device=dev)
        fused.HMC_MAX_DIM = {HIDDEN: 128}  # the kernel at every width, whatever the class default makes of these figures
        assert fused.fused_spec() is not None and fused.fused_spec().hmc, dim
        step = _StepRoute(dim, HIDDEN, device=dev)
        step.net, step.twin = fused.net, fused
        x0 = torch.randn(args.chains, dim, device=dev)
        runs = {
            "fused": ta.HamiltonianMonteCarlo(fused, step_size=0.05, n_leapfrog_steps=args.leapfrog, device=dev),
            "step": ta.HamiltonianMonteCarlo(step, step_size=0.05, n_leapfrog_steps=args.leapfrog, device=dev),
        }
        runs["step"].capture_graph = True  # always the replayed graph, whatever the capture checks make of the wrapper class
        times = {name: [] for name in runs}
        calls0 = _lib.call_counts["ebm_hmc_chain_mlp3_f32"]
        for it in range(args.warmup + args.calls):
            for name, sampler in runs.items():  # alternating, in one process
                ms = _timed(lambda: sampler.sample(x=x0, n_steps=args.steps))
                if it >= args.warmup:
                    times[name].append(ms)
        assert _lib.call_counts["ebm_hmc_chain_mlp3_f32"] == calls0 + args.warmup + args.calls  # the fused route ran the kernel
        rec = {"bench": "mlp3_hmc", "hidden": HIDDEN, "dim": dim, "chains": args.chains, "steps": args.steps,
               "leapfrog": args.leapfrog, "step_gradient": "ebm_energy_grad_mlp3_f32",
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
