"""Cost of per-chain running moments on the MLP energy in one launch: sample_moments() with both opt-ins beside the same steps
through sample() with fused_mlp, and beside what a user had before -- sample_moments() with fused_mlp alone, the step-by-step
recurrence of one launch per transition.

BAOAB and generalized HMC (L = 3) at 2^16 x 32 on MLPEnergy(32, 128) and 65 536 x 2 on MLPEnergy(2, 128), k = 200.
  a  sample_moments, fused_mlp and fused_mlp_moments: ONE launch of ebm_kinetic_moments_mlp_f32
  b  sample(), fused_mlp: ONE launch of ebm_kinetic_mlp_chain_f32 / ebm_ghmc_mlp_chain_f32, the same steps without accumulators
  c  sample_moments, fused_mlp alone: k launches of the plain entry around RunningMoments

The three alternate inside one process; an event pair around every call and, for a and b, the pair around the launch itself
(_lib.timed_events); 2 warm-up and 10 timed calls each; one JSON line per case is appended to
profiles/kinetic_moments_mlp_bench.jsonl (or to the path given as argument): medians with min - max, and the launch ratios a / b (the
cost of the accumulators) and c / a.  --small: a rehearsal size."""

import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torchebm_amd as ta  # noqa: E402
from torchebm_amd import _lib  # noqa: E402

SHAPES = [(1 << 16, 32, 128), (65536, 2, 128)]
K, L, WARMUP, TIMED = 200, 3, 2, 10
ENTRY = "ebm_kinetic_moments_mlp_f32"
PLAIN = {"baoab": "ebm_kinetic_mlp_chain_f32", "ghmc_L3": "ebm_ghmc_mlp_chain_f32"}


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    return start, stop


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def make(which, model, dev):
    if which == "baoab":
        return ta.UnderdampedLangevin(model, step_size=0.1, friction=1.0, temperature=1.0, device=dev)
    return ta.GeneralizedHMC(model, step_size=0.1, n_leapfrog_steps=L, friction=1.0, temperature=1.0, device=dev)


def run(which, n, dim, hidden, k, timed_calls, dev):
    torch.manual_seed(0)
    model = ta.MLPEnergy(dim, hidden, device=dev)
    a, b, c = make(which, model, dev), make(which, model, dev), make(which, model, dev)
    a.fused_mlp = a.fused_mlp_moments = b.fused_mlp = c.fused_mlp = True
    x0 = torch.randn(n, dim, device=dev)
    assert a._route(x0)[0] == "fused_mlp"
    g = torch.Generator(device=dev).manual_seed(0)
    variants = (("a", lambda: a.sample_moments(x=x0, n_steps=k, generator=g)),
                ("b", lambda: b.sample(x=x0, n_steps=k, generator=g)),
                ("c", lambda: c.sample_moments(x=x0, n_steps=k, generator=g)))
    calls = {label: [] for label, _ in variants}
    launches = {"a": [], "b": []}
    for i in range(WARMUP + timed_calls):
        for label, fn in variants:
            # the pairs of the launches inside this call: a and b make one launch, c makes k of the plain entry (not kept)
            _lib.timed_events[ENTRY], _lib.timed_events[PLAIN[which]] = [], []
            start, stop = timed(fn)
            stop.synchronize()
            if i < WARMUP:
                continue
            calls[label].append(start.elapsed_time(stop))
            if label in launches:
                pairs = _lib.timed_events[ENTRY if label == "a" else PLAIN[which]]
                assert len(pairs) == 1, (label, len(pairs))
                launches[label].append(pairs[0][0].elapsed_time(pairs[0][1]))
            else:
                assert len(_lib.timed_events[PLAIN[which]]) == k and not _lib.timed_events[ENTRY]
    _lib.timed_events.pop(ENTRY, None)
    _lib.timed_events.pop(PLAIN[which], None)
    row = {"case": which, "n": n, "dim": dim, "hidden": hidden, "k": k, "warmup": WARMUP, "timed": timed_calls, "unit": "ms",
           "device": torch.cuda.get_device_name(0)}
    for label in calls:
        row[label + "_call"] = spread(calls[label])
    for label in launches:
        row[label + "_launch"] = spread(launches[label])
    row["launch_ratio_a_over_b"] = round(row["a_launch"]["median"] / row["b_launch"]["median"], 4)
    row["ratio_c_call_over_a_launch"] = round(row["c_call"]["median"] / row["a_launch"]["median"], 2)
    row["ratio_c_call_over_a_call"] = round(row["c_call"]["median"] / row["a_call"]["median"], 2)
    return row


def main():
    assert torch.cuda.is_available(), "bench_kinetic_moments_mlp.py needs a GPU"
    dev = torch.device("cuda")
    args = [arg for arg in sys.argv[1:] if arg != "--small"]
    out = args[0] if args else os.path.join(ROOT, "profiles", "kinetic_moments_mlp_bench.jsonl")
    shapes, k, timed_calls = SHAPES, K, TIMED
    if "--small" in sys.argv:
        shapes, k, timed_calls = [(1 << 10, 32, 128), (1 << 10, 2, 128)], 20, 3
    for n, dim, hidden in shapes:
        for which in ("baoab", "ghmc_L3"):
            row = run(which, n, dim, hidden, k, timed_calls, dev)
            print(json.dumps(row), flush=True)
            with open(out, "a") as f:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
