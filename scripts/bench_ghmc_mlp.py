#!/usr/bin/env python3
"""Generalized HMC on the MLP energy in one launch beside the HMC call of the same commit and beside what a user had before
it: one sample() of 20 transitions, L = 3, at two shapes,

  2^16 x 32, MLPEnergy(32, 128)     the benchmark network at dim 32
  65 536 x 2, MLPEnergy(2, 128)     config 5's shape (the two-moons energy)

  fused   GeneralizedHMC.sample() with fused_mlp = True: one ebm_ghmc_mlp_chain_f32 launch of L + 1 evaluations a transition
  hmc     HamiltonianMonteCarlo.sample() on the same rows, the same L and step: one ebm_hmc_chain_f32 launch, whose kernel
          carries its force (L evaluations a transition) -- the figure to read is fused / hmc, (L + 1) / L or less by the code
  eager   the same sampler without the opt-in: torch ops around model / model.gradient, 2 L gradients and two energies a
          transition -- the figure to read is fused / eager, well below 1 by the code

An event pair around every sample() call (and, for the two one-launch routes, the pair around the launch itself from
_lib.timed_events); 2 warm-up and 10 timed calls each, the three alternating inside one process; one JSON line per shape is
appended to profiles/ghmc_mlp_bench.jsonl (medians, spread, the ratios)."""
import json, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchebm_amd as ta
from torchebm_amd import _lib

dev = torch.device("cuda")
SHAPES = [(1 << 16, 32, 128), (65536, 2, 128)]
K, L, REPS, WARM = 20, 3, 10, 2
EPS, GAMMA, TEMP = 0.1, 1.0, 1.0
ENTRY, HMC = "ebm_ghmc_mlp_chain_f32", "ebm_hmc_chain_f32"
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
    fused = ta.GeneralizedHMC(model, step_size=EPS, n_leapfrog_steps=L, friction=GAMMA, temperature=TEMP, device=dev)
    fused.fused_mlp = True
    eager = ta.GeneralizedHMC(model, step_size=EPS, n_leapfrog_steps=L, friction=GAMMA, temperature=TEMP, device=dev)
    hmc = ta.HamiltonianMonteCarlo(model, step_size=EPS, n_leapfrog_steps=L, device=dev)
    rows = torch.randn(n, dim, device=dev)
    assert fused._route(rows)[0] == "fused_mlp" and eager._route(rows)[0] == "eager" and hmc._route(rows, {})[0] == "fused"
    pairs = {"fused": [], "hmc": [], "eager": []}
    for i in range(WARM + REPS):
        if i == WARM:
            torch.cuda.synchronize()
            _lib.timed_events[ENTRY], _lib.timed_events[HMC] = [], []
        got = {"fused": timed(lambda: fused.sample(x=rows, n_steps=K)),
               "hmc": timed(lambda: hmc.sample(x=rows, n_steps=K)),
               "eager": timed(lambda: eager.sample(x=rows, n_steps=K))}
        torch.cuda.synchronize()
        if i >= WARM:
            for key, pair in got.items():
                pairs[key].append(pair[0].elapsed_time(pair[1]))
    torch.cuda.synchronize()
    k_fused = [a.elapsed_time(b) for a, b in _lib.timed_events.pop(ENTRY)]
    k_hmc = [a.elapsed_time(b) for a, b in _lib.timed_events.pop(HMC)]
    rec = {"config": f"MLPEnergy({dim}, {hidden}): {n} chains, {K} transitions, L = {L}, eps = {EPS}, gamma = {GAMMA}, T = {TEMP}"}
    for key, v in pairs.items():
        rec.update({f"{key}_call_ms": median(v), f"{key}_call_ms_min": min(v), f"{key}_call_ms_max": max(v)})
    rec.update({
        "fused_launch_ms": median(k_fused), "fused_launch_ms_min": min(k_fused), "fused_launch_ms_max": max(k_fused),
        "hmc_launch_ms": median(k_hmc), "hmc_launch_ms_min": min(k_hmc), "hmc_launch_ms_max": max(k_hmc),
        "ratio_fused_over_hmc_call": median(pairs["fused"]) / median(pairs["hmc"]),
        "ratio_fused_over_hmc_launch": median(k_fused) / median(k_hmc),
        "ratio_fused_over_eager_call": median(pairs["fused"]) / median(pairs["eager"]),
        "chain_transitions_per_s_fused": n * K / median(k_fused) * 1e3,
        "reps": REPS, "launches_timed": [len(k_fused), len(k_hmc)], "device": torch.cuda.get_device_name(0),
    })
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ghmc_mlp_bench.jsonl")
    for shape in SHAPES:
        rec = run(*shape)
        if not small:
            with open(out, "a") as f:
                f.write(json.dumps(rec) + "\n")
