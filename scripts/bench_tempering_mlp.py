#!/usr/bin/env python3
"""Replica-exchange Langevin on the MLP energy in one launch beside the plain Langevin launch of the same commit on the same rows
and beside what a user had before it: one sample() of 200 steps, eta = 0.01, T = (1, 2, 4, 8), swap_every = 10, at two shapes,

  2^14 ladders x 4 x 32, MLPEnergy(32, 128)     the benchmark network at dim 32
  2^14 ladders x 4 x 2, MLPEnergy(2, 128)       the two-moons energy

  fused    ReplicaExchangeLangevin.sample() with fused_mlp_ladder = True: one ebm_tempering_mlp_chain_f32 launch of one evaluation
           a step and slot (and one more behind the last step), an event every tenth step that evaluates nothing
  langevin (a) LangevinDynamics.sample() on the same 2^16 rows for 200 steps: the launch of ebm_langevin_chain_f32, which runs the
           specialised FAST / THIN units -- the figure to read is the launch ratio fused / langevin, above 1 by the code
  eager    (b) the same sampler without the opt-in, on the GPU: torch ops around model.gradient every step, an autograd energy and
           a Python loop over the pairs at every event -- the figure to read is fused / eager

An event pair around every sample() call and, for the two one-launch routes, the pair around the launch itself (from
_lib.timed_events); 2 warm-up and 10 timed calls each, the three alternating inside one process; one JSON line per shape is
appended to profiles/tempering_mlp_bench.jsonl (medians, spread, the ratios, and whether fused beats eager by more than the
larger of the two min-to-max spreads)."""
import json, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchebm_amd as ta
from torchebm_amd import _lib

dev = torch.device("cuda")
SHAPES = [(1 << 14, 32, 128), (1 << 14, 2, 128)]
K, REPS, WARM = 200, 10, 2
ETA, TEMPS, SWAP_EVERY = 0.01, (1.0, 2.0, 4.0, 8.0), 10
ENTRY, PLAIN = "ebm_tempering_mlp_chain_f32", "ebm_langevin_chain_f32"
small = "--small" in sys.argv  # a rehearsal size
if small:
    SHAPES, REPS, K = [(1 << 8, 32, 128), (1 << 8, 2, 128)], 3, 20


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    return start, stop


def run(n, dim, hidden):
    torch.manual_seed(0)
    R = len(TEMPS)
    model = ta.MLPEnergy(dim, hidden, device=dev)
    kw = dict(step_size=ETA, noise_scale=1.0, temperatures=TEMPS, swap_every=SWAP_EVERY, device=dev)
    fused, eager = ta.ReplicaExchangeLangevin(model, **kw), ta.ReplicaExchangeLangevin(model, **kw)
    fused.fused_mlp_ladder = True
    plain = ta.LangevinDynamics(model, step_size=ETA, noise_scale=1.0, device=dev)
    ladders = torch.randn(n, R, dim, device=dev)
    rows = ladders.view(n * R, dim)
    assert fused._route(ladders)[0] == "fused_mlp" and eager._route(ladders)[0] == "eager"
    pairs = {"fused": [], "langevin": [], "eager": []}
    for i in range(WARM + REPS):
        if i == WARM:
            torch.cuda.synchronize()
            _lib.timed_events[ENTRY], _lib.timed_events[PLAIN] = [], []
        got = {"fused": timed(lambda: fused.sample(x=ladders, n_steps=K)),
               "langevin": timed(lambda: plain.sample(x=rows, n_steps=K)),
               "eager": timed(lambda: eager.sample(x=ladders, n_steps=K))}
        torch.cuda.synchronize()
        if i >= WARM:
            for key, pair in got.items():
                pairs[key].append(pair[0].elapsed_time(pair[1]))
    torch.cuda.synchronize()
    k_fused = [a.elapsed_time(b) for a, b in _lib.timed_events.pop(ENTRY)]
    k_plain = [a.elapsed_time(b) for a, b in _lib.timed_events.pop(PLAIN)]
    assert len(k_fused) == REPS and len(k_plain) == REPS, (len(k_fused), len(k_plain))  # one launch per call on both routes
    rec = {"config": f"MLPEnergy({dim}, {hidden}): {n} ladders x {R}, {K} steps, eta = {ETA}, T = {TEMPS}, swap_every = {SWAP_EVERY}"}
    for key, v in pairs.items():
        rec.update({f"{key}_call_ms": median(v), f"{key}_call_ms_min": min(v), f"{key}_call_ms_max": max(v)})
    spread = max(max(pairs["fused"]) - min(pairs["fused"]), max(pairs["eager"]) - min(pairs["eager"]))
    rec.update({
        "fused_launch_ms": median(k_fused), "fused_launch_ms_min": min(k_fused), "fused_launch_ms_max": max(k_fused),
        "langevin_launch_ms": median(k_plain), "langevin_launch_ms_min": min(k_plain), "langevin_launch_ms_max": max(k_plain),
        "ratio_fused_over_langevin_launch": median(k_fused) / median(k_plain),
        "ratio_fused_over_eager_call": median(pairs["fused"]) / median(pairs["eager"]),
        "larger_min_to_max_spread_ms": spread,
        "fused_faster_than_eager_by_more_than_the_spread": median(pairs["eager"]) - median(pairs["fused"]) > spread,
        "row_steps_per_s_fused": n * R * K / median(k_fused) * 1e3,
        "reps": REPS, "launches_timed": [len(k_fused), len(k_plain)], "device": torch.cuda.get_device_name(0),
    })
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "tempering_mlp_bench.jsonl")
    for shape in SHAPES:
        rec = run(*shape)
        if not small:
            with open(out, "a") as f:
                f.write(json.dumps(rec) + "\n")
