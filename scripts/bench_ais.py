#!/usr/bin/env python3
"""Annealed importance sampling in one launch beside what a user had before it and beside its floor: 2^16 chains x dim 32,
T = 64 linear betas, L = 5, on the double well and on the eight-mode ring mixture of BASELINE config 3.

  fused   AnnealedImportanceSampling.run(): one ebm_ais_chain_f32 launch (event pair around the launch, _lib.timed_events)
  eager   the same estimate through the class's eager route on the GPU (event pair around the whole route): torch ops
  hmc     HamiltonianMonteCarlo.sample doing 64 transitions on the same rows (event pairs around its launches): the same
          evaluations without the path -- the floor

2 warm-up and 10 timed calls each, the three alternating inside one process; one JSON line per energy is appended to
profiles/ais_bench.jsonl (medians, spread, both ratios, the estimate of the last fused call)."""
import json, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchebm_amd as ta
from torchebm_amd import _lib

dev = torch.device("cuda")
N, DIM, T, L, REPS, WARM = 1 << 16, 32, 64, 5, 10, 2
small = "--small" in sys.argv  # a rehearsal size
if small:
    N, REPS = 1 << 10, 3


def median(v):
    return sorted(v)[len(v) // 2]


def run(name, model, eps, base_std):
    ais = ta.AnnealedImportanceSampling(model, n_temperatures=T, schedule="linear", step_size=eps, n_leapfrog_steps=L,
                                        base_std=base_std, device=dev)
    assert ais._route(DIM)[0] == "fused"
    hmc = ta.HamiltonianMonteCarlo(model, step_size=eps, n_leapfrog_steps=L, device=dev)
    rows = base_std * torch.randn(N, DIM, device=dev)
    t_eager, t_hmc, last = [], [], None
    for i in range(WARM + REPS):
        if i == WARM:
            torch.cuda.synchronize()
            _lib.timed_events["ebm_ais_chain_f32"] = []
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
    t_ais = [a.elapsed_time(b) for a, b in _lib.timed_events.pop("ebm_ais_chain_f32")]
    _lib.timed_events.pop("ebm_hmc_chain_f32")
    rec = {
        "config": f"{name}: {N} chains x dim {DIM}, T = {T} linear betas, L = {L}, eps = {eps}, base_std = {base_std}",
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
    recs = [run("double well", ta.DoubleWellModel(device=dev), 0.1, 1.0),
            run("ring_mixture(8, 32)", ta.core.ring_mixture(8, DIM, device=dev), 0.3, 3.0)]
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ais_bench.jsonl")
    if not small:
        with open(out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")
