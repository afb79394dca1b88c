#!/usr/bin/env python3
"""Underdamped Langevin (BAOAB) on the MLP energy in one launch beside the Langevin call of the same commit and beside what a
user had before it: one sample() of k = 20 steps at two shapes,

  2^16 x 32, MLPEnergy(32, 128)     the benchmark network at dim 32
  65 536 x 2, MLPEnergy(2, 128)     config 5's shape (the two-moons energy)

  fused     UnderdampedLangevin.sample() with fused_mlp = True: one ebm_kinetic_mlp_chain_f32 launch of k + 1 evaluations
  langevin  LangevinDynamics.sample() on the same rows: one ebm_langevin_chain_f32 launch of k evaluations (the FAST / THIN
            instantiations) -- the figure to read is fused / langevin
  eager     the same sampler without the opt-in: torch ops around model.gradient, k + 1 gradient launches

An event pair around every sample() call (and, for the two one-launch routes, the pair around the launch itself from
_lib.timed_events); 2 warm-up and 10 timed calls each, the three alternating inside one process; one JSON line per shape is
appended to profiles/kinetic_mlp_bench.jsonl (medians, spread, the ratios)."""
import json, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchebm_amd as ta
from torchebm_amd import _lib

dev = torch.device("cuda")
SHAPES = [(1 << 16, 32, 128), (65536, 2, 128)]
K, REPS, WARM = 20, 10, 2
H, GAMMA, TEMP, ETA = 0.2, 1.0, 1.0, 0.02  # (eta = h^2 / 2: the same distance per step)
ENTRY, LANGEVIN = "ebm_kinetic_mlp_chain_f32", "ebm_langevin_chain_f32"
small = "--small" in sys.argv  # a rehearsal size
if small:
    SHAPES, REPS = [(1 << 10, 32, 128), (1 << 10, 2, 128)], 3


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
    model = ta.MLPEnergy(dim, hidden, device=dev)
    fused = ta.UnderdampedLangevin(model, step_size=H, friction=GAMMA, temperature=TEMP, device=dev)
    fused.fused_mlp = True
    eager = ta.UnderdampedLangevin(model, step_size=H, friction=GAMMA, temperature=TEMP, device=dev)
    langevin = ta.LangevinDynamics(model, step_size=ETA, noise_scale=1.0, device=dev)
    rows = torch.randn(n, dim, device=dev)
    assert fused._route(rows)[0] == "fused_mlp" and eager._route(rows)[0] == "eager" and langevin._route(rows, {})[0] == "fused"
    pairs = {"fused": [], "langevin": [], "eager": []}
    for i in range(WARM + REPS):
        if i == WARM:
            torch.cuda.synchronize()
            _lib.timed_events[ENTRY], _lib.timed_events[LANGEVIN] = [], []
        got = {"fused": timed(lambda: fused.sample(x=rows, n_steps=K)),
               "langevin": timed(lambda: langevin.sample(x=rows, n_steps=K)),
               "eager": timed(lambda: eager.sample(x=rows, n_steps=K))}
        torch.cuda.synchronize()
        if i >= WARM:
            for key, pair in got.items():
                pairs[key].append(pair[0].elapsed_time(pair[1]))
    torch.cuda.synchronize()
    k_fused = [a.elapsed_time(b) for a, b in _lib.timed_events.pop(ENTRY)]
    k_langevin = [a.elapsed_time(b) for a, b in _lib.timed_events.pop(LANGEVIN)]
    rec = {"config": f"MLPEnergy({dim}, {hidden}): {n} chains, k = {K}, h = {H}, gamma = {GAMMA}, T = {TEMP}; Langevin eta = {ETA}"}
    for key, v in pairs.items():
        rec.update({f"{key}_call_ms": median(v), f"{key}_call_ms_min": min(v), f"{key}_call_ms_max": max(v)})
    rec.update({
        "fused_launch_ms": median(k_fused), "fused_launch_ms_min": min(k_fused), "fused_launch_ms_max": max(k_fused),
        "langevin_launch_ms": median(k_langevin), "langevin_launch_ms_min": min(k_langevin), "langevin_launch_ms_max": max(k_langevin),
        "ratio_fused_over_langevin_call": median(pairs["fused"]) / median(pairs["langevin"]),
        "ratio_fused_over_langevin_launch": median(k_fused) / median(k_langevin),
        "ratio_eager_over_fused_call": median(pairs["eager"]) / median(pairs["fused"]),
        "chain_steps_per_s_fused": n * K / median(k_fused) * 1e3,
        "reps": REPS, "launches_timed": [len(k_fused), len(k_langevin)], "device": torch.cuda.get_device_name(0),
    })
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "kinetic_mlp_bench.jsonl")
    for shape in SHAPES:
        rec = run(*shape)
        if not small:
            with open(out, "a") as f:
                f.write(json.dumps(rec) + "\n")
