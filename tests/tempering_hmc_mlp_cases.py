"""Replica-exchange HMC on the MLP energy (include/ebm_hip.h, ebm_tempering_hmc_mlp_chain_f32): the restatement of
tempering_hmc_cases.py as it stands, fed energy and gradient from autograd on the network, the networks, the cases the tests run,
and their inputs.  Shared by test_tempering_hmc_mlp.py (CPU tier) and test_tempering_hmc_mlp_gpu.py; it never calls the package's
sampler."""

import copy
import functools

import torch

from ghmc_mlp_cases import net  # noqa: F401  (the sharpened networks; re-exported for the tests)
from kinetic_mlp_cases import CpuMlpEnergy
from tempering_hmc_cases import MARGIN_BAR, closest_call, draw_inputs, ladder, restate, slot_permutation  # noqa: F401

MAX_SEEDS = 20
MIN_DECISIONS = 3  # accepted and rejected decisions, of the transitions and of the swaps, every case must hold in fp64
THIN = 2
RATIO = {2: 2.0, 4: 2.0, 8: 1.4, 16: 1.25, 32: 1.12}  # T_r = RATIO[R] ** r: the longer ladders step closer, so their pairs swap

# (in_dim, hidden, R, n_ladders, swap_every, n_mh, L): every (HT, DT) -- hidden 64 / 128 at dims 1 .. 32, 33 .. 64, 65 .. 96,
# 97 .. 128 --, every ladder length the entry takes (R = 32: a ladder is a whole wave), the per-element Philox path (dim % 4 != 0)
# and the per-quad one, partial waves (19 x 2 = 38, 5 x 8 = 40, 3 x 16 = 48 rows), several workgroups and a tail (65 x 4 = 260,
# 33 x 4 = 132 rows), both parities on consecutive transitions (swap_every = 1), swap_every = 2, L = 1 and L = 3.
CASES = [
    (2, 64, 4, 65, 1, 4, 1),
    (5, 128, 2, 19, 2, 6, 3),
    (32, 64, 8, 5, 1, 4, 1),
    (33, 128, 16, 3, 1, 4, 3),
    (40, 64, 32, 2, 1, 3, 1),
    (64, 128, 4, 33, 2, 4, 1),
    (65, 64, 2, 19, 1, 3, 3),
    (96, 128, 8, 5, 1, 4, 1),
    (100, 64, 4, 10, 1, 4, 3),
    (128, 64, 2, 19, 2, 4, 1),
    (128, 128, 4, 10, 1, 6, 3),
    (1, 64, 4, 10, 1, 4, 3),
]
# the step sizes of a case, where they are not step_sizes(R) (a case that misses the conditions changes its eps, never the bars)
CASE_EPS = {}


def temperatures(R):
    return tuple(RATIO[R] ** r for r in range(R))


def step_sizes(R):
    """One step size per slot: the hotter slots step a little shorter, so the kernel has to follow the slot's own value."""
    return tuple(1.0 - 0.02 * min(r, 10) for r in range(R))


def energies(cpu):
    """The restatement's energy objects of a CPU network: fp32, and fp64 on a .double() copy."""
    return CpuMlpEnergy(cpu), CpuMlpEnergy(copy.deepcopy(cpu).double())


@functools.lru_cache(maxsize=None)
def case(in_dim, hidden, R, n, swap_every, n_mh, L):
    """Inputs and both restatements (the slot-0 states kept at THIN) of a case, computed once per session and shared (read-only).
    The seed is the first whose fp64 restatement has no MH or swap decision closer than MARGIN_BAR to its threshold and whose fp32
    restatement decides alike; "found" says whether one of the first MAX_SEEDS did."""
    cpu = net(in_dim, hidden)
    e32, e64 = energies(cpu)
    temps = temperatures(R)
    eps = CASE_EPS.get((in_dim, hidden, R, n, swap_every, n_mh, L), step_sizes(R))
    found = False
    for seed in range(MAX_SEEDS):
        x0, z, ua, us = draw_inputs(8100 + seed + in_dim + n, n, R, in_dim, n_mh, swap_every, 1.0)
        ref64 = restate(e64, x0, z, ua, us, eps, L, temps, swap_every, torch.float64, thin=THIN)
        ref32 = None
        if closest_call(ref64) <= MARGIN_BAR:
            continue
        ref32 = restate(e32, x0, z, ua, us, eps, L, temps, swap_every, torch.float32, thin=THIN)
        if torch.equal(ref32["accepted"], ref64["accepted"]) and torch.equal(ref32["mask"], ref64["mask"]):
            found = True
            break
    if ref32 is None:
        ref32 = restate(e32, x0, z, ua, us, eps, L, temps, swap_every, torch.float32, thin=THIN)
    return {"cpu": cpu, "temps": temps, "eps": eps, "L": L, "x0": x0, "z": z, "u_accept": ua, "u_swap": us, "ref32": ref32,
            "ref64": ref64, "seed": seed, "found": found, "shape": (n, R, in_dim), "n_mh": n_mh, "swap_every": swap_every, "thin": THIN}


def swap_attempts(n_events, n, R):
    """[R - 1] attempts of each pair over n_events events on n ladders: pair p is tried at the events of its parity."""
    tried = torch.zeros(R - 1, dtype=torch.long)
    for m in range(n_events):
        tried[m % 2 :: 2] += n
    return tried


def want_swap_counts(mask, n, R):
    """[attempts of each pair | accepts of each pair] from the restatement's swap mask [events, n, R - 1]."""
    return torch.cat([swap_attempts(mask.shape[0], n, R), mask.sum(dim=(0, 1)).long()])


def restatement_errors(c):
    """{key: (fp32 restatement's max error against fp64, max |fp64|)} for the final slot matrix and the kept slot-0 states."""
    out = {}
    for key in ("x", "traj"):
        ref = c["ref64"][key]
        out[key] = ((c["ref32"][key].double() - ref).abs().max().item(), ref.abs().max().item())
    return out


# ---------------------------------------------------------------------------------
# states that cannot move: only the swap events act
# ---------------------------------------------------------------------------------
FROZEN_EVENTS = 6  # swap_every = 1: both parities, three times each


@functools.lru_cache(maxsize=None)
def frozen_case(in_dim, hidden, R, n):
    """eps = 0 in every slot: dH = 0 exactly, every proposal -- the unchanged state -- is accepted, and the final slot matrix is a
    permutation of the start made by the swap decisions alone.  The seed is the first whose fp64 restatement has no swap decision
    within MARGIN_BAR of its threshold, decides like the fp32 one, and both accepts and rejects swaps."""
    cpu = net(in_dim, hidden)
    e32, e64 = energies(cpu)
    temps, eps = temperatures(R), (0.0,) * R
    found = False
    for seed in range(MAX_SEEDS):
        x0, z, ua, us = draw_inputs(8300 + seed + in_dim + n, n, R, in_dim, FROZEN_EVENTS, 1, 1.0)
        ref64 = restate(e64, x0, z, ua, us, eps, 2, temps, 1, torch.float64)
        ref32 = restate(e32, x0, z, ua, us, eps, 2, temps, 1, torch.float32)
        took, tried = int(ref64["mask"].sum()), int(swap_attempts(FROZEN_EVENTS, n, R).sum())
        if ref64["margin"].min().item() > MARGIN_BAR and torch.equal(ref32["mask"], ref64["mask"]) and 0 < took < tried:
            found = True
            break
    return {"cpu": cpu, "temps": temps, "eps": eps, "L": 2, "x0": x0, "z": z, "u_accept": ua, "u_swap": us, "ref32": ref32,
            "ref64": ref64, "seed": seed, "found": found, "shape": (n, R, in_dim), "n_mh": FROZEN_EVENTS, "swap_every": 1}
