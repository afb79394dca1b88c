"""Cost of the step-size adaptation under a mass: ebm_ghmc_adapt_chain_mass_f32 against the unit-mass adapting entry and against
the massed sample() entry, and the host call around each launch.

2^16 chains x 32 dims, 50 transitions, L = 4, on the double well and on ring_mixture(8, 32); the mass is mass_cases' diagonal
exp(U(-log 2, log 4)).  Eight calls alternate in one process, event pairs around each, 2 warm-up and 10 timed rounds, medians; one
JSON line per energy is appended to profiles/ghmc_adapt_mass_bench.jsonl:

  entry_mass     the new entry alone, through _lib.call on preallocated buffers (the state is restored in front of the event pair)
  entry_unit     ebm_ghmc_adapt_chain_f32 alone, likewise
  host_mass      GeneralizedHMC(mass=...).adapt_step_size(apply=False) with the opt-in: the launch, the table, the allocations, the pooling
  host_unit      GeneralizedHMC().adapt_step_size(apply=False)
  frozen_mass    the new entry with n_adapt = 0, gamma = inf, da row 0 == eps
  sample_mass    ebm_ghmc_chain_mass_f32 at the same eps, gamma = inf: the same trajectories as frozen_mass, bit for bit
  frozen_unit    ebm_ghmc_adapt_chain_f32 frozen likewise (against sample_unit, ebm_ghmc_chain_f32)

entry - frozen separates the adaptation (the controller, the per-transition refresh constants, the moving step size) from the
trajectory; host - entry separates the launch from the table, the allocations and the pooling; frozen / sample is what holding the
step size, the drift and the refresh per lane costs the same arithmetic.  No time is a pass/fail bar: the figures to read are the
ratios to the unit-mass adapting entry and to the massed sample() entry of the same commit."""

import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torchebm_amd as ta  # noqa: E402
from torchebm_amd import _lib  # noqa: E402
from torchebm_amd.samplers import adapt  # noqa: E402

N, DIM, N_MH, L, EPS, GAMMA, WARMUP, TIMED = 1 << 16, 32, 50, 4, 0.05, 1.0, 2, 10
MASS_ENTRY, UNIT_ENTRY = "ebm_ghmc_adapt_chain_mass_f32", "ebm_ghmc_adapt_chain_f32"


def once(prepare, fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    prepare()
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def summary(times):
    return {"median": round(statistics.median(times), 4), "min": round(min(times), 4), "max": round(max(times), 4)}


def main():
    assert torch.cuda.is_available(), "bench_adapt_mass.py needs a GPU"
    dev = torch.device("cuda")
    stream = _lib.stream_handle(dev)
    energies = {"double_well": ta.DoubleWellModel(device=dev), "ring_mixture_8": ta.core.ring_mixture(8, DIM, device=dev)}
    out = os.path.join(ROOT, "profiles", "ghmc_adapt_mass_bench.jsonl")
    gm = torch.Generator().manual_seed(4200 + DIM)
    mass = torch.exp(-math.log(2.0) + (math.log(4.0) + math.log(2.0)) * torch.rand(DIM, generator=gm)).to(dev)
    eps_m = EPS * math.sqrt(float(mass.min()))
    for name, model in energies.items():
        spec = model.fused_spec().to_c()
        x0 = torch.randn(N, DIM, device=dev)
        x, v = x0.clone(), torch.empty(N, DIM, device=dev)
        da, alpha = torch.empty(3, N, device=dev), torch.empty(N, device=dev)
        table = adapt.da_table(N_MH).to(dev)
        frozen = {e: torch.stack((torch.full((N,), e), torch.zeros(N), torch.zeros(N))).to(dev) for e in (EPS, eps_m)}
        state = {"offset": 0}

        def restore(da_src=None):
            x.copy_(x0)
            if da_src is not None:
                da.copy_(da_src)

        def adapt_call(entry, eps0, n_adapt, init_da, gamma, m_args):
            state["offset"] += 2 * N_MH + 1
            _lib.call(entry, spec, x.data_ptr(), v.data_ptr(), N, DIM, N_MH, L, eps0, 0.8, math.log(10.0 * eps0), 1e-6, 1e3, n_adapt, init_da,
                      da.data_ptr(), table.data_ptr() if n_adapt else None, None, alpha.data_ptr(), gamma, 1.0, *m_args, 1, 1, None, None,
                      None, None, 1234, state["offset"], stream)

        def sample_call(entry, eps, m_args):
            state["offset"] += 2 * N_MH + 1
            _lib.call(entry, spec, x.data_ptr(), v.data_ptr(), N, DIM, N_MH, L, eps, math.inf, 1.0, *m_args, 1, 1, None, None, None, None, 1234,
                      state["offset"], stream)

        m_args = (_lib.MASS_DIAG, 0.0, mass.data_ptr())
        massed = ta.GeneralizedHMC(model, step_size=eps_m, n_leapfrog_steps=L, friction=GAMMA, temperature=1.0, device=dev, mass=mass)
        massed.fused_adapt_mass = True
        unit = ta.GeneralizedHMC(model, step_size=EPS, n_leapfrog_steps=L, friction=GAMMA, temperature=1.0, device=dev)
        assert adapt.adapt_route(massed, x0, GAMMA)[0] == "fused_mass" and adapt.adapt_route(unit, x0, GAMMA)[0] == "fused"
        g = torch.Generator(device=dev).manual_seed(0)
        calls = {
            "entry_mass": (restore, lambda: adapt_call(MASS_ENTRY, eps_m, N_MH, _lib.DA_INIT, GAMMA, m_args)),
            "entry_unit": (restore, lambda: adapt_call(UNIT_ENTRY, EPS, N_MH, _lib.DA_INIT, GAMMA, ())),
            "host_mass": (lambda: None, lambda: massed.adapt_step_size(x=x0, n_steps=N_MH, generator=g, apply=False)),
            "host_unit": (lambda: None, lambda: unit.adapt_step_size(x=x0, n_steps=N_MH, generator=g, apply=False)),
            "frozen_mass": (lambda: restore(frozen[eps_m]), lambda: adapt_call(MASS_ENTRY, eps_m, 0, 0, math.inf, m_args)),
            "sample_mass": (restore, lambda: sample_call("ebm_ghmc_chain_mass_f32", eps_m, m_args)),
            "frozen_unit": (lambda: restore(frozen[EPS]), lambda: adapt_call(UNIT_ENTRY, EPS, 0, 0, math.inf, ())),
            "sample_unit": (restore, lambda: sample_call("ebm_ghmc_chain_f32", EPS, ())),
        }
        times = {label: [] for label in calls}
        for i in range(WARMUP + TIMED):
            for label, (prepare, fn) in calls.items():  # alternating in one process
                t = once(prepare, fn)
                if i >= WARMUP:
                    times[label].append(t)
        row = {"case": name, "n": N, "dim": DIM, "n_mh": N_MH, "n_leapfrog": L, "eps_unit": EPS, "eps_mass": round(eps_m, 6), "gamma": GAMMA,
               "warmup": WARMUP, "timed": TIMED, "unit": "ms", "device": torch.cuda.get_device_name(0)}
        row.update({label: summary(t) for label, t in times.items()})
        med = lambda label: row[label]["median"]  # noqa: E731
        row["ratio_entry_mass_to_entry_unit"] = round(med("entry_mass") / med("entry_unit"), 3)
        row["ratio_entry_mass_to_sample_mass"] = round(med("entry_mass") / med("sample_mass"), 3)
        row["ratio_frozen_mass_to_sample_mass"] = round(med("frozen_mass") / med("sample_mass"), 3)
        row["ratio_frozen_unit_to_sample_unit"] = round(med("frozen_unit") / med("sample_unit"), 3)
        row["ratio_host_mass_to_entry_mass"] = round(med("host_mass") / med("entry_mass"), 3)
        row["ratio_host_unit_to_entry_unit"] = round(med("host_unit") / med("entry_unit"), 3)
        print(json.dumps(row))
        with open(out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
