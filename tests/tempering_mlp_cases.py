"""Replica-exchange Langevin on the MLP energy (include/ebm_hip.h, ebm_tempering_mlp_chain_f32): the restatement of
tempering_cases.py as it stands, fed energy and gradient from autograd on the network, the networks, the cases the tests run, and
their inputs.  Shared by test_tempering_mlp.py (CPU tier) and test_tempering_mlp_gpu.py; it never calls the package's sampler."""

import copy
import functools

import torch

from ghmc_mlp_cases import net  # noqa: F401  (the sharpened networks; re-exported for the tests)
from kinetic_mlp_cases import CpuMlpEnergy
from tempering_cases import MARGIN_BAR, draw_inputs, ladder, restate  # noqa: F401
from tempering_hmc_cases import slot_permutation  # noqa: F401
from tempering_hmc_mlp_cases import RATIO, swap_attempts, want_swap_counts  # noqa: F401

MAX_SEEDS = 20
MIN_DECISIONS = 3  # accepted and rejected swaps every case must hold in fp64
THIN = 2
ETA, SIGMA = 0.05, 1.0

# (in_dim, hidden, R, n_ladders, swap_every, k): every (HT, DT) -- hidden 64 / 128 at dims 1 .. 32, 33 .. 64, 65 .. 96, 97 .. 128 --,
# every ladder length the entry takes (R = 32: a ladder is a whole wave), the per-element Philox path (dim % 4 != 0) and the
# per-quad one, partial waves (19 x 2 = 38, 5 x 8 = 40, 3 x 16 = 48 rows), several workgroups and a tail (65 x 4 = 260,
# 33 x 4 = 132 rows), both parities on consecutive steps (swap_every = 1), swap_every = 2; k = 3 with THIN = 2 ends on a step
# that is not kept, every other case on a kept step with an event behind it (the kept last step with NO event behind it is
# test_tempering_mlp_gpu.py's own test).
CASES = [
    (2, 64, 4, 65, 1, 4),
    (5, 128, 2, 19, 2, 6),
    (32, 64, 8, 5, 1, 4),
    (33, 128, 16, 3, 1, 4),
    (40, 64, 32, 2, 1, 3),
    (64, 128, 4, 33, 2, 4),
    (65, 64, 2, 19, 1, 3),
    (96, 128, 8, 5, 1, 4),
    (100, 64, 4, 10, 1, 4),
    (128, 64, 2, 19, 2, 4),
    (128, 128, 4, 10, 1, 6),
    (1, 64, 4, 10, 1, 4),
]
# the step size of a case, where it is not ETA (a case that misses the conditions changes its eta, never the bars)
CASE_ETA = {}


def temperatures(R):
    return tuple(RATIO[R] ** r for r in range(R))


def energies(cpu):
    """The restatement's energy objects of a CPU network: fp32, and fp64 on a .double() copy."""
    return CpuMlpEnergy(cpu), CpuMlpEnergy(copy.deepcopy(cpu).double())


def closest_call(ref):
    """The smallest margin of a run's swap decisions (inf when it decided nothing)."""
    return ref["margin"].min().item() if ref["margin"].numel() else float("inf")


@functools.lru_cache(maxsize=None)
def case(in_dim, hidden, R, n, swap_every, k):
    """Inputs and both restatements (the slot-0 states kept at THIN) of a case, computed once per session and shared (read-only).
    The seed is the first whose fp64 restatement has no swap decision closer than MARGIN_BAR to its threshold, whose fp32
    restatement decides alike and which holds at least MIN_DECISIONS accepted and as many rejected swaps; "found" says whether
    one of the first MAX_SEEDS did."""
    cpu = net(in_dim, hidden)
    e32, e64 = energies(cpu)
    temps = temperatures(R)
    eta = CASE_ETA.get((in_dim, hidden, R, n, swap_every, k), ETA)
    tried = int(swap_attempts(k // swap_every, n, R).sum())
    found = False
    for seed in range(MAX_SEEDS):
        x0, z, u = draw_inputs(8500 + seed + in_dim + n, n, R, in_dim, k, swap_every, 1.0)
        ref64 = restate(e64, x0, z, u, eta, SIGMA, temps, swap_every, torch.float64, thin=THIN)
        ref32 = None
        if closest_call(ref64) <= MARGIN_BAR:
            continue
        ref32 = restate(e32, x0, z, u, eta, SIGMA, temps, swap_every, torch.float32, thin=THIN)
        took = int(ref64["mask"].sum())
        if torch.equal(ref32["mask"], ref64["mask"]) and took >= MIN_DECISIONS and tried - took >= MIN_DECISIONS:
            found = True
            break
    if ref32 is None:
        ref32 = restate(e32, x0, z, u, eta, SIGMA, temps, swap_every, torch.float32, thin=THIN)
    return {"cpu": cpu, "temps": temps, "eta": eta, "sigma": SIGMA, "x0": x0, "z": z, "u": u, "ref32": ref32, "ref64": ref64,
            "seed": seed, "found": found, "shape": (n, R, in_dim), "k": k, "swap_every": swap_every, "thin": THIN}


def restatement_errors(c):
    """{key: (fp32 restatement's max error against fp64, max |fp64|)} for the final slot matrix and the kept slot-0 states."""
    out = {}
    for key in ("x", "traj"):
        ref = c["ref64"][key]
        out[key] = ((c["ref32"][key].double() - ref).abs().max().item(), ref.abs().max().item())
    return out


# ---------------------------------------------------------------------------------
# a kept last step with no event behind it
# ---------------------------------------------------------------------------------
TAIL_K, TAIL_THIN, TAIL_SWAP_EVERY = 4, 2, 3  # the one event follows step 2; step 3 is kept and nothing is due behind it but the store


@functools.lru_cache(maxsize=None)
def tail_case(in_dim, hidden, R, n):
    """The first seed whose fp64 restatement has no swap decision within MARGIN_BAR of its threshold, decides like the fp32 one and
    both accepts and rejects swaps."""
    cpu = net(in_dim, hidden)
    e32, e64 = energies(cpu)
    temps = temperatures(R)
    found = False
    for seed in range(MAX_SEEDS):
        x0, z, u = draw_inputs(8900 + seed + in_dim + n, n, R, in_dim, TAIL_K, TAIL_SWAP_EVERY, 1.0)
        ref64 = restate(e64, x0, z, u, ETA, SIGMA, temps, TAIL_SWAP_EVERY, torch.float64, thin=TAIL_THIN)
        ref32 = restate(e32, x0, z, u, ETA, SIGMA, temps, TAIL_SWAP_EVERY, torch.float32, thin=TAIL_THIN)
        took, tried = int(ref64["mask"].sum()), int(swap_attempts(1, n, R).sum())
        if closest_call(ref64) > MARGIN_BAR and torch.equal(ref32["mask"], ref64["mask"]) and 0 < took < tried:
            found = True
            break
    return {"cpu": cpu, "temps": temps, "eta": ETA, "sigma": SIGMA, "x0": x0, "z": z, "u": u, "ref32": ref32, "ref64": ref64,
            "seed": seed, "found": found, "shape": (n, R, in_dim), "k": TAIL_K, "swap_every": TAIL_SWAP_EVERY, "thin": TAIL_THIN}


# ---------------------------------------------------------------------------------
# states that cannot move: only the swap events act
# ---------------------------------------------------------------------------------
FROZEN_EVENTS = 6  # swap_every = 1: both parities, three times each


@functools.lru_cache(maxsize=None)
def frozen_case(in_dim, hidden, R, n):
    """eta = sqrt_eta = 0: x - 0 g + coef (z 0) is x bit for bit, and the final slot matrix is a permutation of the start made by
    the swap decisions alone.  The seed is the first whose fp64 restatement has no swap decision within MARGIN_BAR of its
    threshold, decides like the fp32 one, and both accepts and rejects swaps."""
    cpu = net(in_dim, hidden)
    e32, e64 = energies(cpu)
    temps = temperatures(R)
    found = False
    for seed in range(MAX_SEEDS):
        x0, z, u = draw_inputs(8700 + seed + in_dim + n, n, R, in_dim, FROZEN_EVENTS, 1, 1.0)
        ref64 = restate(e64, x0, z, u, 0.0, SIGMA, temps, 1, torch.float64)
        ref32 = restate(e32, x0, z, u, 0.0, SIGMA, temps, 1, torch.float32)
        took, tried = int(ref64["mask"].sum()), int(swap_attempts(FROZEN_EVENTS, n, R).sum())
        if ref64["margin"].min().item() > MARGIN_BAR and torch.equal(ref32["mask"], ref64["mask"]) and 0 < took < tried:
            found = True
            break
    return {"cpu": cpu, "temps": temps, "eta": 0.0, "sigma": SIGMA, "x0": x0, "z": z, "u": u, "ref32": ref32, "ref64": ref64,
            "seed": seed, "found": found, "shape": (n, R, in_dim), "k": FROZEN_EVENTS, "swap_every": 1, "thin": None}
