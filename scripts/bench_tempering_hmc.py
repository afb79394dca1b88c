#!/usr/bin/env python3
"""Replica-exchange HMC beside plain HMC on the same rows: 2^16 ladders x 4 slots x dim 32 (the double well, and the
eight-mode ring mixture of BASELINE config 3), L = 10, 20 transitions, a swap event every 2, against
HamiltonianMonteCarlo.sample on [2^18, 32] for 20 transitions.  Times are event pairs around the one launch of each call
(_lib.timed_events), the two samplers alternating inside one process; one JSON line per energy is appended to
profiles/tempering_hmc_bench.jsonl."""
import json, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchebm_amd as ta
from torchebm_amd import _lib

dev = torch.device("cuda")
LADDERS, R, DIM, K, L, SWAP_EVERY, REPS, WARM = 1 << 16, 4, 32, 20, 10, 2, 10, 2
EPS = 0.05
small = "--small" in sys.argv  # a rehearsal size
if small:
    LADDERS, REPS = 1 << 10, 3


def median(v):
    return sorted(v)[len(v) // 2]


def run(name, model):
    rows = torch.randn(LADDERS * R, DIM, device=dev)
    pt = ta.ReplicaExchangeHMC(model, step_size=EPS, n_leapfrog_steps=L, temperatures=(1.0, 2.0, 4.0, 8.0), swap_every=SWAP_EVERY,
                               device=dev)
    hmc = ta.HamiltonianMonteCarlo(model, step_size=EPS, n_leapfrog_steps=L, device=dev)
    ladders = rows.view(LADDERS, R, DIM)
    swap_acc = mh_acc = None
    for i in range(WARM + REPS):
        if i == WARM:
            torch.cuda.synchronize()
            _lib.timed_events["ebm_tempering_hmc_chain_f32"] = []
            _lib.timed_events["ebm_hmc_chain_f32"] = []
        if i == WARM + REPS - 1:
            _, diag = pt.sample(x=ladders, n_steps=K, return_replicas=True, return_diagnostics=True)
            swap_acc, mh_acc = diag["swap_acceptance"].tolist(), diag["acceptance_rate"].tolist()
        else:
            pt.sample(x=ladders, n_steps=K, return_replicas=True)
        hmc.sample(x=rows, n_steps=K)
    torch.cuda.synchronize()
    t_pt = [a.elapsed_time(b) for a, b in _lib.timed_events.pop("ebm_tempering_hmc_chain_f32")]
    t_hmc = [a.elapsed_time(b) for a, b in _lib.timed_events.pop("ebm_hmc_chain_f32")]
    rec = {
        "config": f"{name}: {LADDERS} ladders x {R} slots x dim {DIM}, {K} transitions, L = {L}, eps = {EPS}, swap_every = {SWAP_EVERY}",
        "tempering_hmc_ms": median(t_pt), "tempering_hmc_ms_min": min(t_pt), "tempering_hmc_ms_max": max(t_pt),
        "hmc_ms": median(t_hmc), "hmc_ms_min": min(t_hmc), "hmc_ms_max": max(t_hmc),
        "ratio_tempering_hmc_over_hmc": median(t_pt) / median(t_hmc),
        "row_transitions_per_s_tempering_hmc": LADDERS * R * K / median(t_pt) * 1e3,
        "row_transitions_per_s_hmc": LADDERS * R * K / median(t_hmc) * 1e3,
        "swap_acceptance": swap_acc, "acceptance_rate": mh_acc, "reps": REPS, "launches_timed": [len(t_pt), len(t_hmc)],
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    recs = [run("double well", ta.DoubleWellModel(device=dev)), run("ring_mixture(8, 32)", ta.core.ring_mixture(8, DIM, device=dev))]
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "tempering_hmc_bench.jsonl")
    if not small:
        with open(out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")
