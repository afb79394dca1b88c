#!/usr/bin/env python3
"""Replica-exchange HMC on the MLP energy in one launch beside the generalized-HMC launch of the same commit on the same rows and
beside what a user had before it: one sample() of 20 transitions, L = 3, eps = 0.1, T = (1, 2, 4, 8), swap_every = 2, at two
shapes,

  2^14 ladders x 4 x 32, MLPEnergy(32, 128)     the benchmark network at dim 32
  2^14 ladders x 4 x 2, MLPEnergy(2, 128)       the two-moons energy

  fused   ReplicaExchangeHMC.sample() with fused_mlp = True: one ebm_tempering_hmc_mlp_chain_f32 launch of L + 1 evaluations a
          transition and slot, an event every second transition that evaluates nothing
  ghmc    (a) the launch of ebm_ghmc_mlp_chain_f32 at gamma = inf on the same 2^16 rows with the same L and step: the same
          transition without the ladder -- the figure to read is the launch ratio fused / ghmc, close to 1 by the code
  eager   (b) the same sampler without the opt-in, on the GPU: torch ops around model / model.gradient, 2 L gradients and two
          energies a transition and a Python loop over the pairs at every event -- the figure to read is fused / eager

An event pair around every sample() call and, for the two one-launch routes, the pair around the launch itself (from
_lib.timed_events); 2 warm-up and 10 timed calls each, the three alternating inside one process; one JSON line per shape is
appended to profiles/tempering_hmc_mlp_bench.jsonl (medians, spread, the ratios)."""
import json, math, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchebm_amd as ta
from torchebm_amd import _lib

dev = torch.device("cuda")
SHAPES = [(1 << 14, 32, 128), (1 << 14, 2, 128)]
K, L, REPS, WARM = 20, 3, 10, 2
EPS, TEMPS, SWAP_EVERY = 0.1, (1.0, 2.0, 4.0, 8.0), 2
ENTRY, GHMC = "ebm_tempering_hmc_mlp_chain_f32", "ebm_ghmc_mlp_chain_f32"
small = "--small" in sys.argv  # a rehearsal size
if small:
    SHAPES, REPS = [(1 << 8, 32, 128), (1 << 8, 2, 128)], 3


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
    kw = dict(step_size=EPS, n_leapfrog_steps=L, temperatures=TEMPS, swap_every=SWAP_EVERY, device=dev)
    fused, eager = ta.ReplicaExchangeHMC(model, **kw), ta.ReplicaExchangeHMC(model, **kw)
    fused.fused_mlp = True
    ghmc = ta.GeneralizedHMC(model, step_size=EPS, n_leapfrog_steps=L, friction=math.inf, temperature=1.0, device=dev)
    ghmc.fused_mlp = True
    ladders = torch.randn(n, R, dim, device=dev)
    rows = ladders.view(n * R, dim)
    assert fused._route(ladders)[0] == "fused_mlp" and eager._route(ladders)[0] == "eager" and ghmc._route(rows)[0] == "fused_mlp"
    pairs = {"fused": [], "ghmc": [], "eager": []}
    for i in range(WARM + REPS):
        if i == WARM:
            torch.cuda.synchronize()
            _lib.timed_events[ENTRY], _lib.timed_events[GHMC] = [], []
        got = {"fused": timed(lambda: fused.sample(x=ladders, n_steps=K)),
               "ghmc": timed(lambda: ghmc.sample(x=rows, n_steps=K)),
               "eager": timed(lambda: eager.sample(x=ladders, n_steps=K))}
        torch.cuda.synchronize()
        if i >= WARM:
            for key, pair in got.items():
                pairs[key].append(pair[0].elapsed_time(pair[1]))
    torch.cuda.synchronize()
    k_fused = [a.elapsed_time(b) for a, b in _lib.timed_events.pop(ENTRY)]
    k_ghmc = [a.elapsed_time(b) for a, b in _lib.timed_events.pop(GHMC)]
    rec = {"config": f"MLPEnergy({dim}, {hidden}): {n} ladders x {R}, {K} transitions, L = {L}, eps = {EPS}, T = {TEMPS}, "
                     f"swap_every = {SWAP_EVERY}"}
    for key, v in pairs.items():
        rec.update({f"{key}_call_ms": median(v), f"{key}_call_ms_min": min(v), f"{key}_call_ms_max": max(v)})
    rec.update({
        "fused_launch_ms": median(k_fused), "fused_launch_ms_min": min(k_fused), "fused_launch_ms_max": max(k_fused),
        "ghmc_launch_ms": median(k_ghmc), "ghmc_launch_ms_min": min(k_ghmc), "ghmc_launch_ms_max": max(k_ghmc),
        "ratio_fused_over_ghmc_launch": median(k_fused) / median(k_ghmc),
        "ratio_fused_over_eager_call": median(pairs["fused"]) / median(pairs["eager"]),
        "row_transitions_per_s_fused": n * R * K / median(k_fused) * 1e3,
        "reps": REPS, "launches_timed": [len(k_fused), len(k_ghmc)], "device": torch.cuda.get_device_name(0),
    })
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "tempering_hmc_mlp_bench.jsonl")
    for shape in SHAPES:
        rec = run(*shape)
        if not small:
            with open(out, "a") as f:
                f.write(json.dumps(rec) + "\n")
