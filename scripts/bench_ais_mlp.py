#!/usr/bin/env python3
"""Annealed importance sampling on the MLP energy in one launch beside what a user had before it and beside its floor:
2^14 chains, MLPEnergy(32, 128), T = 64 linear betas, L = 5.

  fused   AnnealedImportanceSampling.run() with fused_mlp = True: one ebm_ais_mlp_chain_f32 launch (event pair around the
          launch, _lib.timed_events)
  eager   the same estimate through the class's eager route on the GPU (event pair around the whole route): torch ops, the
          gradient one HIP launch per call
  hmc     HamiltonianMonteCarlo.sample doing 64 transitions of the same L on the same rows (event pairs around its launches):
          the same L + 1 evaluations per transition without the path and the weight -- the floor

2 warm-up and 10 timed calls each, the three alternating inside one process; one JSON line is appended to
profiles/ais_mlp_bench.jsonl (medians, spread, both ratios, the estimate of the last fused call)."""
import json, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchebm_amd as ta
from torchebm_amd import _lib

dev = torch.device("cuda")
N, DIM, HIDDEN, T, L, REPS, WARM = 1 << 14, 32, 128, 64, 5, 10, 2
EPS, BASE_STD = 0.2, 1.0
ENTRY = "ebm_ais_mlp_chain_f32"
small = "--small" in sys.argv  # a rehearsal size
if small:
    N, REPS = 1 << 10, 3


def median(v):
    return sorted(v)[len(v) // 2]


def run():
    torch.manual_seed(0)
    model = ta.MLPEnergy(DIM, HIDDEN, device=dev)
    ais = ta.AnnealedImportanceSampling(model, n_temperatures=T, schedule="linear", step_size=EPS, n_leapfrog_steps=L,
                                        base_std=BASE_STD, device=dev)
    ais.fused_mlp = True
    assert ais._route(DIM)[0] == "fused_mlp"
    hmc = ta.HamiltonianMonteCarlo(model, step_size=EPS, n_leapfrog_steps=L, device=dev)
    rows = BASE_STD * torch.randn(N, DIM, device=dev)
    t_eager, t_hmc, last = [], [], None
    for i in range(WARM + REPS):
        if i == WARM:
            torch.cuda.synchronize()
            _lib.timed_events[ENTRY] = []
            _lib.timed_events["ebm_hmc_chain_f32"] = []
        last = ais.run(N, DIM)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        ais._run_eager(N, DIM, None)
        stop.record()
        seen = len(_lib.timed_events.get("ebm_hmc_chain_f32", []))
        hmc.sample(x=rows, n_steps=T)
        torch.cuda.synchronize()
        if i >= WARM:
            t_eager.append(start.elapsed_time(stop))
            t_hmc.append(sum(a.elapsed_time(b) for a, b in _lib.timed_events["ebm_hmc_chain_f32"][seen:]))
    t_ais = [a.elapsed_time(b) for a, b in _lib.timed_events.pop(ENTRY)]
    _lib.timed_events.pop("ebm_hmc_chain_f32")
    rec = {
        "config": f"MLPEnergy({DIM}, {HIDDEN}): {N} chains, T = {T} linear betas, L = {L}, eps = {EPS}, base_std = {BASE_STD}",
        "ais_fused_ms": median(t_ais), "ais_fused_ms_min": min(t_ais), "ais_fused_ms_max": max(t_ais),
        "ais_eager_ms": median(t_eager), "ais_eager_ms_min": min(t_eager), "ais_eager_ms_max": max(t_eager),
        "hmc_ms": median(t_hmc), "hmc_ms_min": min(t_hmc), "hmc_ms_max": max(t_hmc),
        "ratio_eager_over_fused": median(t_eager) / median(t_ais),
        "ratio_fused_over_hmc": median(t_ais) / median(t_hmc),
        "chain_transitions_per_s_fused": N * T / median(t_ais) * 1e3,
        "log_z": last.log_z, "log_z_stderr": last.log_z_stderr, "ess": last.ess, "acceptance_rate_mean": last.acceptance_rate.mean().item(),
        "reps": REPS, "launches_timed": len(t_ais), "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    rec = run()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ais_mlp_bench.jsonl")
    if not small:
        with open(out, "a") as f:
            f.write(json.dumps(rec) + "\n")
